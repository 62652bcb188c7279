// iso_cell_check.cpp -- the per-cell routine of vdn_isosurface (varden_amd/csrc/iso_cell.h) held without a GPU: every mask of every Kuhn tetrahedron on random values
// (above + below volume = the cell's, every normal towards the not-above side, every vertex the bits of the canonical crossing of its edge), a plane through one cell against
// the analytic section and cut, nodes equal to iso, non-finite nodes, and the node means with and without face values.  Built with -fsanitize=address,undefined by
// tests/test_isosurface_cpu.py.
#include "iso_cell.h"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fails++; if (fails < 40) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Tri { double p[3][3]; };
struct Cell { int ntri; IsoSums S; std::vector<Tri> tri; };

static Cell run(const double (&q)[8], const double (&xlo)[3], const double (&xhi)[3], double iso, double vtet) {
  Cell c;
  c.ntri = iso_cell(q, xlo, xhi, iso, vtet, c.S, [&](const double (&p0)[3], const double (&p1)[3], const double (&p2)[3]) {
    Tri t; memcpy(t.p[0], p0, sizeof p0); memcpy(t.p[1], p1, sizeof p1); memcpy(t.p[2], p2, sizeof p2); c.tri.push_back(t);
  });
  CHECK(c.ntri == iso_count(q, iso), "iso_count gives %d, iso_cell %d", iso_count(q, iso), c.ntri);
  CHECK(c.ntri == ISO_NONFINITE || c.ntri == (int)c.tri.size(), "%d triangles returned, %zu emitted", c.ntri, c.tri.size());
  return c;
}
static bool same_bits(double a, double b) { return memcmp(&a, &b, 8) == 0; }
static double corner_x(int c, int d, const double (&xlo)[3], const double (&xhi)[3]) { return ((c >> d) & 1) ? xhi[d] : xlo[d]; }

// the axis orders written out, independent of iso_tet
static const int ORDER[6][3] = { { 0, 1, 2 }, { 0, 2, 1 }, { 1, 0, 2 }, { 1, 2, 0 }, { 2, 0, 1 }, { 2, 1, 0 } };

static void random_cells() {
  std::mt19937_64 rng(12345);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  bool seen[6][16] = {};
  const double xlo[3] = { 3 * 0.25, 5 * 0.125, 7 * 0.5 }, xhi[3] = { 4 * 0.25, 6 * 0.125, 8 * 0.5 }, h[3] = { 0.25, 0.125, 0.5 };
  const double vol = (h[0] * h[1]) * h[2], vtet = vol / 6.0;
  for (int trial = 0; trial < 4000; trial++) {
    double q[8], nq[8];
    const double iso = U(rng);
    // every corner above or below by a random margin: all 256 sign patterns turn up, and with them every mask of every tetrahedron
    for (int c = 0; c < 8; c++) { q[c] = (rng() & 1) ? iso + 0.01 + U(rng) : iso - 0.01 - U(rng); nq[c] = -q[c]; }
    const Cell A = run(q, xlo, xhi, iso, vtet), B = run(nq, xlo, xhi, -iso, vtet);
    CHECK(std::fabs((A.S.vol + B.S.vol) - vol) <= 16 * std::numeric_limits<double>::epsilon() * vol, "above %.17g + below %.17g != %.17g", A.S.vol, B.S.vol, vol);
    CHECK(A.ntri == B.ntri, "a field and its negative: %d and %d triangles", A.ntri, B.ntri);
    CHECK(std::fabs(A.S.area - B.S.area) <= 64 * std::numeric_limits<double>::epsilon() * (A.S.area + 1e-300), "a field and its negative: area %.17g and %.17g", A.S.area, B.S.area);
    // the canonical crossings of the 19 edges of the triangulation: corners a, b with the bits of a inside those of b
    std::vector<std::vector<double>> cross;
    for (int a = 0; a < 8; a++) for (int b = 0; b < 8; b++) {
      if (a == b || (a & b) != a) continue;
      const bool aa = q[a] > iso, ab = q[b] > iso;
      if (aa == ab) continue;
      const int lo = aa ? b : a, hi = aa ? a : b;
      const double t = (iso - q[lo]) / (q[hi] - q[lo]);
      std::vector<double> p(3);
      for (int d = 0; d < 3; d++) { const double xa = corner_x(lo, d, xlo, xhi), xb = corner_x(hi, d, xlo, xhi); p[d] = xa + t * (xb - xa); }
      cross.push_back(p);
    }
    size_t next = 0;
    double area = 0.0;
    for (int n = 0; n < 6; n++) {
      const int *o = ORDER[n];
      const int c[4] = { 0, 1 << o[0], (1 << o[0]) | (1 << o[1]), 7 };
      int mask = 0, nab = 0;
      for (int v = 0; v < 4; v++) if (q[c[v]] > iso) { mask |= 1 << v; nab++; }
      seen[n][mask] = true;
      const int want = nab == 2 ? 2 : (nab == 1 || nab == 3) ? 1 : 0;
      // the gradient of the tetrahedron's linear interpolant: its edges v0 v1, v1 v2, v2 v3 run along the axes
      double g[3];
      for (int e = 0; e < 3; e++) g[o[e]] = (q[c[e + 1]] - q[c[e]]) / h[o[e]];
      for (int k = 0; k < want; k++, next++) {
        if (next >= A.tri.size()) { CHECK(false, "tetrahedron %d mask %d: triangle missing", n, mask); break; }
        const Tri &T = A.tri[next];
        double e1[3], e2[3];
        for (int d = 0; d < 3; d++) { e1[d] = T.p[1][d] - T.p[0][d]; e2[d] = T.p[2][d] - T.p[0][d]; }
        const double cr[3] = { e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0] };
        const double dot = -(cr[0] * g[0] + cr[1] * g[1] + cr[2] * g[2]);
        CHECK(dot > 0.0, "tetrahedron %d mask %d triangle %d: normal . (-grad q) = %g", n, mask, k, dot);
        area += 0.5 * std::sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]);
        for (int v = 0; v < 3; v++) {
          bool found = false;
          for (const auto &p : cross) found = found || (same_bits(p[0], T.p[v][0]) && same_bits(p[1], T.p[v][1]) && same_bits(p[2], T.p[v][2]));
          CHECK(found, "tetrahedron %d mask %d triangle %d vertex %d is not the canonical crossing of an edge", n, mask, k, v);
          // ... and lies inside the tetrahedron's box
          for (int d = 0; d < 3; d++) CHECK(T.p[v][d] >= xlo[d] && T.p[v][d] <= xhi[d], "a vertex outside the cell");
        }
      }
    }
    CHECK(next == A.tri.size(), "%zu triangles expected from the masks, %zu emitted", next, A.tri.size());
    CHECK(std::fabs(area - A.S.area) <= 64 * std::numeric_limits<double>::epsilon() * (area + 1e-300), "area %.17g, from the triangles %.17g", A.S.area, area);
  }
  for (int n = 0; n < 6; n++) for (int m = 0; m < 16; m++) CHECK(seen[n][m], "tetrahedron %d mask %d never came up", n, m);
  // the tetrahedra of iso_tet are the ones written out above
  for (int n = 0; n < 6; n++) {
    int c1, c2; bool pos;
    iso_tet(n, c1, c2, pos);
    const int *o = ORDER[n];
    const int inv = (o[0] > o[1]) + (o[0] > o[2]) + (o[1] > o[2]);
    CHECK(c1 == (1 << o[0]) && c2 == ((1 << o[0]) | (1 << o[1])) && pos == (inv % 2 == 0), "iso_tet(%d): corners %d, %d, positive %d", n, c1, c2, (int)pos);
  }
}

// q = sum of w_d x_d / h_d + b at the corners of the cell [x0, x0 + h]
static void plane(const double (&w)[3], double iso, double want_area, double want_above, const char *name) {
  const double h[3] = { 0.25, 0.5, 0.125 }, xlo[3] = { 2 * h[0], 3 * h[1], 5 * h[2] }, xhi[3] = { 3 * h[0], 4 * h[1], 6 * h[2] };
  double q[8];
  for (int c = 0; c < 8; c++) q[c] = w[0] * (c & 1) + w[1] * ((c >> 1) & 1) + w[2] * ((c >> 2) & 1);
  const double vol = (h[0] * h[1]) * h[2];
  const Cell A = run(q, xlo, xhi, iso, vol / 6.0);
  const double eps = std::numeric_limits<double>::epsilon();
  CHECK(std::fabs(A.S.area - want_area) <= 64 * eps * want_area, "%s: area %.17g, analytic %.17g", name, A.S.area, want_area);
  CHECK(std::fabs(A.S.vol - want_above) <= 64 * eps * vol, "%s: volume above %.17g, analytic %.17g", name, A.S.vol, want_above);
  // the area vector of a plane section is area * (-grad q / |grad q|)
  double g[3], gn = 0.0;
  for (int d = 0; d < 3; d++) { g[d] = w[d] / h[d]; gn += g[d] * g[d]; }
  gn = std::sqrt(gn);
  for (int d = 0; d < 3; d++) CHECK(std::fabs(A.S.av[d] + want_area * g[d] / gn) <= 64 * eps * want_area, "%s: area_vec[%d] = %.17g", name, d, A.S.av[d]);
}

static void planes() {
  const double h[3] = { 0.25, 0.5, 0.125 }, vol = (h[0] * h[1]) * h[2];
  { const double w[3] = { 1, 0, 0 }; plane(w, 0.25, h[1] * h[2], 0.75 * vol, "q = x"); }
  { const double w[3] = { 0, 0, -1 }; plane(w, -0.625, h[0] * h[1], 0.625 * vol, "q = -z"); }
  { const double w[3] = { 1, 1, 0 }; plane(w, 0.5, h[2] * std::sqrt(0.25 * h[0] * h[0] + 0.25 * h[1] * h[1]), vol - 0.125 * vol, "q = x + y"); }
  {
    const double w[3] = { 1, 1, 1 }, a[3] = { 0.5 * h[0], 0.5 * h[1], 0.5 * h[2] };
    const double cr[3] = { a[1] * a[2], a[0] * a[2], a[0] * a[1] };
    plane(w, 0.5, 0.5 * std::sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]), vol - vol / 48.0, "q = x + y + z, a corner cut off");
  }
  {   // the middle section of the cube along the diagonal: a hexagon; the volume above is half the cell
    const double w[3] = { 1, 1, 1 };
    const double cr[3] = { h[1] * h[2], h[0] * h[2], h[0] * h[1] };
    plane(w, 1.5, 0.75 * std::sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]), 0.5 * vol, "q = x + y + z, the middle");
  }
}

static void edge_values() {
  const double xlo[3] = { 0, 0, 0 }, xhi[3] = { 1, 1, 1 }, inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  // every node equal to iso: nothing is above, nothing is divided
  { double q[8]; for (double &v : q) v = 0.5; const Cell A = run(q, xlo, xhi, 0.5, 1.0 / 6.0); CHECK(A.ntri == 0 && A.S.vol == 0.0 && A.S.area == 0.0, "all nodes equal iso"); }
  // some equal, some above, some below, every pattern over {below, equal, above}^8 of a few corners: finite output, t in [0, 1]
  for (int pat = 0; pat < 6561; pat++) {
    double q[8]; int r = pat;
    for (int c = 0; c < 8; c++, r /= 3) q[c] = 0.5 + 0.25 * (r % 3 - 1);
    const Cell A = run(q, xlo, xhi, 0.5, 1.0 / 6.0);
    bool any_above = false, any_not = false;
    for (double v : q) { any_above = any_above || v > 0.5; any_not = any_not || !(v > 0.5); }
    CHECK((A.ntri > 0) == (any_above && any_not), "pattern %d: %d triangles", pat, A.ntri);
    CHECK(std::isfinite(A.S.area) && std::isfinite(A.S.vol) && A.S.vol >= 0.0 && A.S.vol <= 1.0 + 1e-15, "pattern %d: area %g volume %g", pat, A.S.area, A.S.vol);
    for (const Tri &T : A.tri) for (int v = 0; v < 3; v++) for (int d = 0; d < 3; d++) CHECK(T.p[v][d] >= 0.0 && T.p[v][d] <= 1.0, "pattern %d: a vertex at %g", pat, T.p[v][d]);
  }
  // all above: the whole cell, six times V_tet added in order
  { double q[8]; for (double &v : q) v = 1.0; const Cell A = run(q, xlo, xhi, 0.5, 1.0 / 6.0); double v = 0.0; for (int n = 0; n < 6; n++) v = v + 1.0 / 6.0;
    CHECK(A.ntri == 0 && same_bits(A.S.vol, v), "all above: volume %.17g", A.S.vol); }
  // a node that is not finite: the cell emits nothing and adds nothing
  for (double bad : { nan, inf, -inf }) for (int c = 0; c < 8; c++) {
    double q[8] = { 0, 1, 0, 1, 0, 1, 0, 1 }; q[c] = bad;
    const Cell A = run(q, xlo, xhi, 0.5, 1.0 / 6.0);
    CHECK(A.ntri == ISO_NONFINITE && A.tri.empty() && A.S.vol == 0.0 && A.S.area == 0.0, "a non-finite node %d", c);
  }
}

static void nodes() {
  std::mt19937_64 rng(99);
  std::uniform_real_distribution<double> U(-1.0, 1.0);
  for (int trial = 0; trial < 256; trial++) {
    double a[27], q[8];
    for (double &v : a) v = U(rng);
    bool flo[3], fhi[3];
    for (int d = 0; d < 3; d++) { flo[d] = (trial >> d) & 1; fhi[d] = (trial >> (3 + d)) & 1; }
    iso_nodes(a, flo, fhi, q);
    for (int c = 0; c < 8; c++) {
      // written out: x, then y, then z; a face node takes the ghost value alone
      auto A = [&](int i, int j, int k) { return a[i + 3 * j + 9 * k]; };
      auto mean = [&](double lo, double hi, int d, int side) { return side == 0 ? (flo[d] ? lo : 0.5 * lo + 0.5 * hi) : (fhi[d] ? hi : 0.5 * lo + 0.5 * hi); };
      const int cx = c & 1, cy = (c >> 1) & 1, cz = (c >> 2) & 1;
      double my[2];
      for (int kk = 0; kk < 2; kk++) {
        double mx[2];
        for (int jj = 0; jj < 2; jj++) mx[jj] = mean(A(cx, cy + jj, cz + kk), A(cx + 1, cy + jj, cz + kk), 0, cx);
        my[kk] = mean(mx[0], mx[1], 1, cy);
      }
      const double want = mean(my[0], my[1], 2, cz);
      CHECK(same_bits(want, q[c]), "node %d (faces %d): %.17g, written out %.17g", c, trial, q[c], want);
    }
  }
}

// --cases: every case (tetrahedron n, mask m) on the unit cube with vertex values +-1 (the cell's other corners -1), the triangles the header emits for that
// tetrahedron, one per line: n m k and the nine coordinates.  tests/test_isosurface_cpu.py holds them against the numpy restatement, whose turns come from the rule
static void print_cases() {
  const double xlo[3] = { 0, 0, 0 }, xhi[3] = { 1, 1, 1 };
  for (int n = 0; n < 6; n++) for (int m = 1; m < 15; m++) {
    const int *o = ORDER[n];
    const int c[4] = { 0, 1 << o[0], (1 << o[0]) | (1 << o[1]), 7 };
    double q[8];
    for (double &v : q) v = -1.0;
    for (int v = 0; v < 4; v++) q[c[v]] = ((m >> v) & 1) ? 1.0 : -1.0;
    const Cell A = run(q, xlo, xhi, 0.0, 1.0 / 6.0);
    size_t first = 0;
    for (int e = 0; e < n; e++) {
      int c1, c2; bool pos;
      iso_tet(e, c1, c2, pos);
      const int nab = iso_bits4(iso_tet_mask(q, 0.0, c1, c2));
      first += nab == 2 ? 2 : (nab == 1 || nab == 3) ? 1 : 0;
    }
    const int nab = iso_bits4(m), cnt = nab == 2 ? 2 : 1;
    for (int k = 0; k < cnt; k++) {
      const Tri &T = A.tri[first + k];
      printf("%d %d %d", n, m, k);
      for (int v = 0; v < 3; v++) for (int d = 0; d < 3; d++) printf(" %.17g", T.p[v][d]);
      printf("\n");
    }
  }
}

int main(int argc, char **argv) {
  if (argc > 1 && strcmp(argv[1], "--cases") == 0) { print_cases(); return 0; }
  random_cells();
  planes();
  edge_values();
  nodes();
  if (fails) { printf("%d failure(s)\n", fails); return 1; }
  printf("OK iso_cell.h\n");
  return 0;
}
