// The tile arithmetic of varden_amd/csrc/nd_lds_plan.h, without a GPU and without the library: for every extent triple out of 16, 24, .. 64 every fine node
// 0 .. n is owned by exactly one tile and every coarse node 0 .. n/2 is restricted by exactly one; the three working regions of the down kernel nest as the
// sweeps need them (each one node inside the one it reads) and lie inside the LDS boxes, as do the sigma cells, the residual entries the full weighting
// reads and the up kernel's reads; extents 8, 20 and 72 are refused.  Built and run by tests/test_nd_lds_plan_cpu.py.
#include "nd_lds_plan.h"
#include <cstdio>
#include <vector>

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_bad++; fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static bool inside(NdLdsRange r, int lo, int count) { return r.lo >= lo && r.hi <= lo + count - 1 && r.lo <= r.hi; }

// one axis of n cells: ranges, nesting, boxes
static void check_axis(int n) {
  const int T = nd_lds_tiles(n);
  CHECK(T * ND_LDS_T == n && T >= 2, "n %d", n);
  std::vector<int> fine(n + 1, 0), coarse(n / 2 + 1, 0);
  for (int a = 0; a < T; a++) {
    const NdLdsRange of = nd_lds_own_fine(n, a), oc = nd_lds_own_coarse(n, a);
    for (int i = of.lo; i <= of.hi; i++) { CHECK(i >= 0 && i <= n, "n %d tile %d fine %d", n, a, i); if (i >= 0 && i <= n) fine[i]++; }
    for (int i = oc.lo; i <= oc.hi; i++) { CHECK(i >= 0 && i <= n / 2, "n %d tile %d coarse %d", n, a, i); if (i >= 0 && i <= n / 2) coarse[i]++; }
    CHECK(oc.lo * 2 == of.lo && oc.hi * 2 >= of.hi - 1 && oc.hi * 2 <= of.hi, "n %d tile %d: the coarse nodes lie under the fine ones", n, a);
    CHECK(oc.hi - oc.lo + 1 <= ND_LDS_T / 2 + 1 && of.hi - of.lo + 1 <= ND_LDS_T + 1, "n %d tile %d: owned counts", n, a);
    // the down kernel
    const NdLdsRange s1 = nd_lds_sweep1(a), s2 = nd_lds_sweep2(a), rs = nd_lds_resid(n, a), rb = nd_lds_resbox(a);
    const int b0 = nd_lds_box_lo(a), g0 = nd_lds_sig_lo(a);
    CHECK(inside(s1, b0, ND_LDS_BOX) && inside(s2, b0, ND_LDS_BOX) && inside(rs, b0, ND_LDS_BOX) && inside(rb, b0, ND_LDS_BOX), "n %d tile %d: regions in the box", n, a);
    CHECK(s2.lo - 1 >= s1.lo && s2.hi + 1 <= s1.hi, "n %d tile %d: sweep 2 reads sweep 1", n, a);
    // the residual reads sweep 2 one node around; beyond sweep 2's region only nodes outside the level (zero) may be read
    CHECK(rs.lo - 1 >= s2.lo && (rs.hi + 1 <= s2.hi || rs.hi + 1 > n) && rs.hi + 1 <= b0 + ND_LDS_BOX - 1, "n %d tile %d: the residual reads sweep 2", n, a);
    CHECK(of.lo >= s2.lo && of.hi <= s2.hi, "n %d tile %d: the owned nodes are swept twice", n, a);
    // the full weighting of coarse node I reads the residual at 2I-1 .. 2I+1: computed, or outside the level, and stored either way
    CHECK(2 * oc.lo - 1 >= rs.lo && (2 * oc.hi + 1 <= rs.hi || 2 * oc.hi + 1 > n) && inside(NdLdsRange{ 2 * oc.lo - 1, 2 * oc.hi + 1 }, rb.lo, rb.hi - rb.lo + 1), "n %d tile %d: full weighting", n, a);
    // sigma: the cells i-1, i around every node i of the box
    CHECK(g0 <= s1.lo - 1 && s1.hi <= g0 + ND_LDS_SIG - 1, "n %d tile %d: sigma box", n, a);
    // the up kernel: the owned nodes grown by one in the phi box, their cells in the sigma box
    const int u0 = nd_lds_ubox_lo(a), ug = nd_lds_usig_lo(a);
    CHECK(inside(NdLdsRange{ of.lo - 1, of.hi + 1 }, u0, ND_LDS_UBOX), "n %d tile %d: up box", n, a);
    CHECK(ug <= of.lo - 1 && of.hi <= ug + ND_LDS_USIG - 1, "n %d tile %d: up sigma box", n, a);
  }
  for (int i = 0; i <= n; i++) CHECK(fine[i] == 1, "n %d: fine node %d owned %d times", n, i, fine[i]);
  for (int i = 0; i <= n / 2; i++) CHECK(coarse[i] == 1, "n %d: coarse node %d restricted %d times", n, i, coarse[i]);
}

int main() {
  for (int n = ND_LDS_NMIN; n <= ND_LDS_NMAX; n += ND_LDS_T) { CHECK(nd_lds_extent_ok(n), "extent %d", n); check_axis(n); }
  // the triples: ownership is the product of the axes' -- counted in full all the same
  long triples = 0;
  for (int nx = 16; nx <= 64; nx += 8) for (int ny = 16; ny <= 64; ny += 8) for (int nz = 16; nz <= 64; nz += 8) {
    const int n[3] = { nx, ny, nz };
    std::vector<unsigned char> fine((size_t)(nx + 1) * (ny + 1) * (nz + 1), 0), coarse((size_t)(nx / 2 + 1) * (ny / 2 + 1) * (nz / 2 + 1), 0);
    for (int c = 0; c < nd_lds_tiles(nz); c++) for (int b = 0; b < nd_lds_tiles(ny); b++) for (int a = 0; a < nd_lds_tiles(nx); a++) {
      const int t[3] = { a, b, c };
      NdLdsRange f[3], q[3];
      for (int d = 0; d < 3; d++) { f[d] = nd_lds_own_fine(n[d], t[d]); q[d] = nd_lds_own_coarse(n[d], t[d]); }
      for (int k = f[2].lo; k <= f[2].hi; k++) for (int j = f[1].lo; j <= f[1].hi; j++) for (int i = f[0].lo; i <= f[0].hi; i++) fine[i + (size_t)(nx + 1) * (j + (size_t)(ny + 1) * k)]++;
      for (int k = q[2].lo; k <= q[2].hi; k++) for (int j = q[1].lo; j <= q[1].hi; j++) for (int i = q[0].lo; i <= q[0].hi; i++) coarse[i + (size_t)(nx / 2 + 1) * (j + (size_t)(ny / 2 + 1) * k)]++;
    }
    long badf = 0, badc = 0;
    for (unsigned char v : fine) badf += v != 1;
    for (unsigned char v : coarse) badc += v != 1;
    CHECK(badf == 0 && badc == 0, "%d x %d x %d: %ld fine and %ld coarse nodes not owned exactly once", nx, ny, nz, badf, badc);
    triples++;
  }
  CHECK(triples == 343, "%ld triples", triples);
  // refused: too narrow, no multiple of the tile, too wide (and the neighbours of the limits)
  const int refused[] = { 0, 4, 8, 12, 20, 28, 36, 63, 65, 72, 128 };
  for (int n : refused) CHECK(!nd_lds_extent_ok(n), "extent %d must be refused", n);
  // the LDS the boxes take: two phi boxes and sigma going down, one of each going up, within 64 KB
  CHECK((2 * ND_LDS_BOX * ND_LDS_BOX * ND_LDS_BOX + ND_LDS_SIG * ND_LDS_SIG * ND_LDS_SIG) * 8 <= 65536, "LDS of the down kernel");
  CHECK((ND_LDS_UBOX * ND_LDS_UBOX * ND_LDS_UBOX + ND_LDS_USIG * ND_LDS_USIG * ND_LDS_USIG) * 8 <= 65536, "LDS of the up kernel");
  if (g_bad) { printf("FAILED %d checks\n", g_bad); return 1; }
  printf("OK %ld triples\n", triples);
  return 0;
}
