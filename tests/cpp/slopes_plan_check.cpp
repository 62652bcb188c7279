// slopes_plan_check.cpp -- holds varden_amd/csrc/slopes_plan.h without a GPU: for a set of boxes it walks every thread of every workgroup the way
// kk_slopes_pr does (the same clamps, the same LDS slots) and checks that
//   * every cell of the range (the box grown by one) is stored exactly once, every plane is in exactly one k-chunk,
//   * every 16-byte load and store is aligned and inside its allocation,
//   * the four rows a lane reads from the staged plane were written by exactly one thread each and hold the pair and the row it wants,
//   * the staged planes fit the workgroup's LDS budget,
//   * a box of odd width is refused (it keeps kk_slopes_my).
// Built by tests/test_slopes_plan_cpu.py, plain and under the address / undefined-behaviour sanitizers.  Prints "OK ..." and returns 0.
#include "slopes_plan.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Arr { int a[3], n[3]; long sc; };        // an allocation: lowest index and extent per direction, component stride
static Arr grown(const int lo[3], const int hi[3], int g) {
  Arr f;
  for (int d = 0; d < 3; d++) { f.a[d] = lo[d] - g; f.n[d] = hi[d] - lo[d] + 1 + 2 * g; }
  f.sc = (long)f.n[0] * f.n[1] * f.n[2];
  return f;
}
static int clampi(int v, int a, int b) { return std::min(std::max(v, a), b); }

// returns 1 when the box takes the pair form, 0 when it is refused
static int check_box(const char *name, const int n[3], const int lo[3], int wg_target, bool expect_pair) {
  int hi[3], rlo[3], rhi[3];
  for (int d = 0; d < 3; d++) { hi[d] = lo[d] + n[d] - 1; rlo[d] = lo[d] - 1; rhi[d] = hi[d] + 1; }
  const Arr s = grown(lo, hi, 3), sl = grown(lo, hi, 1);
  const int nx = n[0] + 2, ny = n[1] + 2, nz = n[2] + 2;
  const SlopesLayout Ls = { (long)rlo[0] - s.a[0], s.n[0], s.sc, 0 }, Ll = { (long)rlo[0] - sl.a[0], sl.n[0], sl.sc, 0 };
  const bool pair = slopes_pair_ok(nx, rlo[0] - (lo[0] - 3), hi[0] + 3 - rhi[0], Ls, Ll);
  CHECK(pair == expect_pair, "%s: pair form %d, expected %d", name, (int)pair, (int)expect_pair);
  if (!pair) return 0;
  // a misaligned base or an odd stride refuses
  SlopesLayout bad = Ls; bad.base = 8; CHECK(!slopes_pair_ok(nx, 2, 2, bad, Ll), "%s: base", name);
  bad = Ll; bad.n0++; CHECK(!slopes_pair_ok(nx, 2, 2, Ls, bad), "%s: stride", name);
  bad = Ls; bad.off0++; CHECK(!slopes_pair_ok(nx, 2, 2, bad, Ll), "%s: offset", name);

  const SlopesPlan P = slopes_plan(nx, ny, nz, wg_target);
  const int slots = (SLP_WAVES + 4) * 64, threads = 64 * SLP_WAVES;
  CHECK(slopes_lds_bytes() <= SLP_LDS_BUDGET && slots * 16 * 2 == slopes_lds_bytes(), "%s: LDS %d", name, slopes_lds_bytes());
  CHECK(P.tiles == P.gxm * P.gy + P.gyr && P.tiles >= 1 && P.chunks >= 1 && P.klen >= 1, "%s: plan", name);
  // planes: chunk c takes k0 = rlo + c klen .. min(k0 + klen - 1, rhi)
  std::vector<int> kcov(nz, 0);
  for (int c = 0; c < P.chunks; c++) {
    const int k0 = rlo[2] + c * P.klen, k1 = std::min(k0 + P.klen - 1, rhi[2]);
    CHECK(k0 <= k1, "%s: empty chunk %d", name, c);
    for (int k = k0; k <= k1; k++) kcov[k - rlo[2]]++;
  }
  for (int k = 0; k < nz; k++) CHECK(kcov[k] == 1, "%s: plane %d in %d chunks", name, k, kcov[k]);

  std::vector<int> cov((size_t)nx * ny, 0);
  std::vector<int> wr(slots), scol(slots), srow(slots);
  for (int t = 0; t < P.tiles; t++) {
    int lw, pair0, by;
    slopes_tile(P, t, lw, pair0, by);
    CHECK(lw >= 2 && lw <= 6 && 4 * (1 << lw) <= threads, "%s: lw %d", name, lw);
    const int W = 1 << lw, rows = SLP_WAVES * (64 >> lw), j0 = rlo[1] + by * rows;
    std::fill(wr.begin(), wr.end(), 0);
    // pass 1: what every thread loads and stages
    for (int tid = 0; tid < threads; tid++) {
      int pl, rr, hrow, hslot;
      slopes_lane(lw, tid, pl, rr);
      const bool hal = slopes_halo(lw, tid, hrow, hslot);
      const int i = rlo[0] + 2 * (pair0 + pl - 1), j = j0 + rr;
      const int ic = clampi(i, lo[0] - 3, hi[0] + 2), jc = clampi(j, lo[1] - 3, hi[1] + 3);
      const long off = ic - s.a[0];
      CHECK((off & 1) == 0 && off >= 0 && off + 1 < s.n[0], "%s: load column %ld of %d", name, off, s.n[0]);
      CHECK(jc - s.a[1] >= 0 && jc - s.a[1] < s.n[1], "%s: load row", name);
      CHECK(((off + (long)s.n[0] * (jc - s.a[1])) & 1) == 0 && (((long)s.n[0] * s.n[1]) & 1) == 0 && (s.sc & 1) == 0, "%s: load alignment", name);
      const int o0 = (rr + 2) * W + pl;
      CHECK(o0 - 2 * W >= 0 && o0 + 2 * W < slots, "%s: slot %d", name, o0);
      wr[o0]++; scol[o0] = ic; srow[o0] = jc;
      if (hal) {
        const int jh = clampi(j0 + hrow, lo[1] - 3, hi[1] + 3), oh = hslot * W + pl;
        CHECK(oh >= 0 && oh < slots, "%s: halo slot %d", name, oh);
        CHECK(jh - s.a[1] >= 0 && jh - s.a[1] < s.n[1], "%s: halo row", name);
        wr[oh]++; scol[oh] = ic; srow[oh] = jh;
      }
    }
    // pass 2: what the owners read and store
    for (int tid = 0; tid < threads; tid++) {
      int pl, rr;
      const bool own_l = slopes_lane(lw, tid, pl, rr);
      const int i = rlo[0] + 2 * (pair0 + pl - 1), j = j0 + rr;
      if (!(own_l && i <= rhi[0] && j <= rhi[1])) continue;
      CHECK(i >= rlo[0] && i + 1 <= rhi[0] && j >= rlo[1], "%s: owner outside the range", name);
      CHECK(tid >= 1 && tid + 1 < threads && ((tid - 1) >> 6) == (tid >> 6) && ((tid + 1) >> 6) == (tid >> 6), "%s: x-neighbours in another wave", name);
      // the lanes next door hold the pairs next door, unclamped
      for (int dl = -1; dl <= 1; dl += 2) {
        int pl2, rr2;
        slopes_lane(lw, tid + dl, pl2, rr2);
        const int i2 = rlo[0] + 2 * (pair0 + pl2 - 1);
        CHECK(rr2 == rr && i2 == i + 2 * dl && clampi(i2, lo[0] - 3, hi[0] + 2) == i2, "%s: lane %d's neighbour", name, tid);
      }
      const int o0 = (rr + 2) * W + pl, dj[4] = { -2, -1, 1, 2 };
      for (int q = 0; q < 4; q++) {
        const int o = o0 + dj[q] * W;
        CHECK(wr[o] == 1 && scol[o] == i && srow[o] == j + dj[q], "%s: tile %d thread %d reads row %+d: slot written %d times, holds (%d, %d), wants (%d, %d)", name, t, tid, dj[q],
              wr[o], scol[o], srow[o], i, j + dj[q]);
      }
      CHECK(wr[o0] == 1 && scol[o0] == i && srow[o0] == j, "%s: own slot", name);
      const long so = i - sl.a[0];
      CHECK((so & 1) == 0 && so >= 0 && so + 1 < sl.n[0] && (sl.n[0] & 1) == 0 && (sl.sc & 1) == 0 && j - sl.a[1] < sl.n[1], "%s: store", name);
      cov[(size_t)(j - rlo[1]) * nx + (i - rlo[0])]++; cov[(size_t)(j - rlo[1]) * nx + (i + 1 - rlo[0])]++;
    }
  }
  long badc = 0;
  for (size_t q = 0; q < cov.size(); q++) badc += cov[q] != 1;
  CHECK(badc == 0, "%s: %ld cells of a plane not stored exactly once", name, badc);
  return 1;
}

int main() {
  const int R = SLP_WAVES, z[3] = { 0, 0, 0 }, c357[3] = { 3, 5, 7 }, right[3] = { 64, 0, 0 };
  const struct { const char *name; int n[3]; const int *lo; bool pair; } cases[] = {
    { "8^3", { 8, 8, 8 }, z, true }, { "124x4x8", { 124, 4, 8 }, z, true }, { "126x7x12", { 126, 7, 12 }, z, true }, { "132x(R+1)x20", { 132, R + 1, 20 }, z, true },
    { "61x5x9", { 61, 5, 9 }, z, false }, { "10x6x8 at (3,5,7)", { 10, 6, 8 }, c357, true }, { "64 wide", { 64, 16, 16 }, z, true }, { "62 wide beside it", { 62, 16, 16 }, right, true },
    { "16^3", { 16, 16, 16 }, z, true }, { "256^3", { 256, 256, 256 }, z, true }, { "512^3", { 512, 512, 512 }, z, true }, { "4^3", { 4, 4, 4 }, z, true }, { "60x3x5", { 60, 3, 5 }, z, true },
  };
  int npair = 0, n = 0;
  for (const auto &c : cases)
    for (int target : { 1, 512, 4096 }) { npair += check_box(c.name, c.n, c.lo, target, c.pair); n++; }
  if (fails) { printf("%d checks failed\n", fails); return 1; }
  printf("OK %d plans, %d in the pair form, %d waves per workgroup, %d bytes of LDS per workgroup\n", n, npair, SLP_WAVES, slopes_lds_bytes());
  return 0;
}
