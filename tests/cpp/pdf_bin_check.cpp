// pdf_bin_check.cpp -- the slot rule of vdn_pdf / vdn_pdf2 (varden_amd/csrc/pdf_bin.h) held without a GPU on the values where it can go wrong: exactly lo, exactly
// hi, the largest double below hi (the clamp), -0 with lo = 0, +-Inf, NaN, nbins = 1 and 256, a width that is no power of two, and a range so wide that q - lo
// overflows.  Every slot is also compared with the rule written out independently (edges by long double).  Built with -fsanitize=address,undefined by
// tests/test_pdf_cpu.py -- a float-to-int conversion out of range would stop it.
#include "pdf_bin.h"
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static int slot(double q, double lo, double hi, int nbins) { return pdf_slot(q, lo, hi, pdf_width(lo, hi, nbins), nbins); }

// what every axis must satisfy whatever its width
static void check_axis(double lo, double hi, int nbins) {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double w = pdf_width(lo, hi, nbins);
  CHECK(w > 0.0 && w == (hi - lo) / nbins, "[%g, %g) / %d: width %g", lo, hi, nbins, w);
  CHECK(slot(lo, lo, hi, nbins) == 1, "[%g, %g) / %d: lo itself lies in slot %d", lo, hi, nbins, slot(lo, lo, hi, nbins));
  CHECK(slot(hi, lo, hi, nbins) == nbins + 1, "[%g, %g) / %d: hi itself lies in slot %d", lo, hi, nbins, slot(hi, lo, hi, nbins));
  CHECK(slot(std::nextafter(hi, -inf), lo, hi, nbins) == nbins, "[%g, %g) / %d: the last value below hi lies in slot %d", lo, hi, nbins, slot(std::nextafter(hi, -inf), lo, hi, nbins));
  CHECK(slot(std::nextafter(lo, -inf), lo, hi, nbins) == 0, "[%g, %g) / %d: the last value below lo", lo, hi, nbins);
  CHECK(slot(inf, lo, hi, nbins) == nbins + 1 && slot(-inf, lo, hi, nbins) == 0, "[%g, %g) / %d: +-Inf", lo, hi, nbins);
  CHECK(slot(DBL_MAX, lo, hi, nbins) == nbins + 1 && slot(-DBL_MAX, lo, hi, nbins) == 0, "[%g, %g) / %d: +-DBL_MAX", lo, hi, nbins);
  CHECK(slot(nan, lo, hi, nbins) == PDF_NO_SLOT && slot(-nan, lo, hi, nbins) == PDF_NO_SLOT, "[%g, %g) / %d: NaN", lo, hi, nbins);
  // a sweep: the slot never decreases, stays in 1 .. nbins inside the range, and is the written-out rule
  int last = 0;
  const int steps = 4 * nbins + 7;
  for (int i = -3; i <= steps + 3; i++) {
    const double q = lo + (hi - lo) * ((double)i / steps);
    const int s = slot(q, lo, hi, nbins);
    int want;
    if (q < lo) want = 0;
    else if (q >= hi) want = nbins + 1;
    else { const double m = std::floor((q - lo) / w); want = 1 + (m > nbins - 1 ? nbins - 1 : (int)m); }
    CHECK(s == want, "[%g, %g) / %d: q = %.17g lies in slot %d, the rule gives %d", lo, hi, nbins, q, s, want);
    CHECK(s >= last, "[%g, %g) / %d: the slot falls from %d to %d at q = %.17g", lo, hi, nbins, last, s, q);
    CHECK(!(q >= lo && q < hi) || (s >= 1 && s <= nbins), "[%g, %g) / %d: q = %.17g inside the range lies in slot %d", lo, hi, nbins, q, s);
    last = s;
  }
  // every bin's own lower edge lo + m w, where it is below hi, lies in bin m or m - 1 (the edge itself is rounded) -- never further off
  for (int m = 0; m < nbins; m++) {
    const double e = lo + m * w;
    if (!(e >= lo && e < hi)) continue;
    const int s = slot(e, lo, hi, nbins);
    CHECK(s == 1 + m || s == m || s == 2 + m, "[%g, %g) / %d: edge %d = %.17g lies in slot %d", lo, hi, nbins, m, e, s);
  }
}

int main() {
  const double inf = std::numeric_limits<double>::infinity();
  // -0 with lo = 0 is not below lo: bin 0; the smallest negative number is
  CHECK(slot(-0.0, 0.0, 1.0, 4) == 1, "-0 with lo = 0 lies in slot %d", slot(-0.0, 0.0, 1.0, 4));
  CHECK(slot(-0.0, -0.0, 1.0, 4) == 1 && slot(0.0, -0.0, 1.0, 4) == 1, "+-0 with lo = -0");
  CHECK(slot(-4.9406564584124654e-324, 0.0, 1.0, 4) == 0, "the smallest negative number with lo = 0");
  // exact arithmetic: a power-of-two width, every edge is the first value of its bin
  for (int m = 0; m < 8; m++) {
    CHECK(slot(m * 0.125, 0.0, 1.0, 8) == 1 + m, "edge %d of [0, 1) / 8 lies in slot %d", m, slot(m * 0.125, 0.0, 1.0, 8));
    CHECK(slot(std::nextafter(m * 0.125, -inf), 0.0, 1.0, 8) == m, "just below edge %d of [0, 1) / 8 lies in slot %d", m, slot(std::nextafter(m * 0.125, -inf), 0.0, 1.0, 8));
  }
  // nbins = 1: everything inside is bin 0
  CHECK(slot(0.3, 0.0, 1.0, 1) == 1 && slot(0.0, 0.0, 1.0, 1) == 1 && slot(std::nextafter(1.0, 0.0), 0.0, 1.0, 1) == 1 && slot(1.0, 0.0, 1.0, 1) == 2, "nbins = 1");
  // the clamp is needed: here (q - lo) / w rounds up to nbins for the last value below hi
  {
    const double lo = 0.0, hi = 0.7; const int nb = 7;
    const double q = std::nextafter(hi, -inf), w = pdf_width(lo, hi, nb);
    CHECK(slot(q, lo, hi, nb) == nb, "the last value below 0.7 on [0, 0.7) / 7 lies in slot %d (quotient %.17g)", slot(q, lo, hi, nb), (q - lo) / w);
  }
  // a range whose extent overflows is refused by the library (w is not finite); one that is only just finite still works
  check_axis(-8.0e307, 8.0e307, 3);
  check_axis(0.0, 1.0, 1); check_axis(0.0, 1.0, 256); check_axis(-1.0, 1.0, 7); check_axis(0.9, 2.1, 256); check_axis(-0.3, 0.7, 64); check_axis(1.0, 3.0, 3);
  check_axis(1e-300, 3e-300, 5); check_axis(-3.0, -1.0, 64); check_axis(0.0, 0.1, 10); check_axis(-1.25, 1.0 / 3.0, 255);
  if (fails) { printf("%d failure(s)\n", fails); return 1; }
  printf("OK pdf_bin.h\n");
  return 0;
}
