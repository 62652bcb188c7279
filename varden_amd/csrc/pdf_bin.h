// pdf_bin.h -- the slot of a value on a uniform axis: the one rule of vdn_pdf / vdn_pdf2 (pdf.hip; include/varden_amd.h states it).  No HIP, no library type: hipcc
// compiles it for the kernels, plain g++ for tests/cpp/pdf_bin_check.cpp, and the tests restate it in numpy; the three agree on every bit.
//
// An axis {lo, hi, nbins} has the width w = (hi - lo) / nbins, formed ONCE on the host in double (pdf_width), and nbins + 2 slots: slot 0 "below", slots 1 .. nbins
// the bins, slot nbins + 1 "above".  In this order:
//   1.  q != q     no slot (PDF_NO_SLOT): the cell counts in nan_cells and in nothing else
//   2.  q <  lo    slot 0
//   3.  q >= hi    slot nbins + 1
//   4.  otherwise  m = floor((q - lo) / w) -- a true division, never a multiplication by 1 / w, and never contracted --, clamped to nbins - 1; the slot is 1 + m
// +-Inf fall out of rules 2 and 3; -0 with lo = 0 is not below lo and lands in bin 0; the clamp catches the values just below hi whose quotient rounds up to nbins.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PDF_HD __host__ __device__
#else
#define PDF_HD
#endif

constexpr int PDF_NO_SLOT = -1;

inline double pdf_width(double lo, double hi, int nbins) { return (hi - lo) / (double)nbins; }

PDF_HD inline int pdf_slot(double q, double lo, double hi, double w, int nbins) {
  if (q != q) return PDF_NO_SLOT;
  if (q < lo) return 0;
  if (q >= hi) return nbins + 1;
  const double m = floor((q - lo) / w);                   // >= 0; compared as a double before it becomes an int: a huge quotient (or Inf, where q - lo overflows) is clamped too
  return 1 + (m >= (double)(nbins - 1) ? nbins - 1 : (int)m);
}
