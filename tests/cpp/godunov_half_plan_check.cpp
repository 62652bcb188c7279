// godunov_half_plan_check.cpp -- holds the half-workgroup grid of varden_amd/csrc/godunov_plan.h (god_grid_half, kk_mk_F_mh) without a GPU.  Over face ranges
// from 1 x 1 x 1 to 300 x 70 x 40 and both segment widths (16 and 32 lanes) it walks every thread of every 64 x THY workgroup the way the march does
// (god_thread, god_cell, god_planes with THY waves) and checks that
//   * no lane of a wave is left over, and every (lane, row) of a workgroup is held by one thread;
//   * every cell (i, j) of the range is owned by exactly one (workgroup, thread) and nothing outside it is owned;
//   * everything a workgroup computes -- its footprint (god_footprint) -- is what its threads compute, and stays inside the range grown by one cell
//     wherever the workgroup owns a cell at that end (a remainder tile reaches further: its loads are clamped, its lanes there own nothing);
//   * the chunks cover nz exactly once, with the chunk rule (512 workgroup slots) and with a forced count;
//   * the form chooser returns today's form when the box is below god_half_min or the switch is off, and whenever today's form cannot be the column
//     grid's (no update, no power-of-two spacing, no face with a rule, an inflow face, a batched launch); where it returns the half form it is in the
//     instantiation list, and differs from today's form in cols and half alone.
// Built plain and under the address / undefined-behaviour sanitizers.  Prints "OK ..." and returns 0.
#include "godunov_plan.h"
#include <algorithm>
#include <cstdio>
#include <vector>

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static long n_wg = 0;
static void check_range(int nx, int ny, int nz, int W) {
  const int lo[3] = { 3, -5, 7 }, hi[3] = { lo[0] + nx - 1, lo[1] + ny - 1, lo[2] + nz - 1 };
  const GodSeg S = god_seg(W, THY);
  CHECK(S.W == W && S.rows == THY * (64 / W) && S.ownx == W - 2 && S.owny == S.rows - 2 && S.W * S.rows == 64 * THY, "W %d: segments", W);
  for (int kch : { 0, 1, 2, 5, 16 }) {
    const GodGrid G = god_grid_half(nx, ny, nz, W, kch);
    CHECK(G.segw == W && G.g[0] == (nx + S.ownx - 1) / S.ownx && G.g[1] == (ny + S.owny - 1) / S.owny, "W %d (%d, %d, %d): grid %d x %d", W, nx, ny, nz, G.g[0], G.g[1]);
    CHECK(G.klen >= 1 && G.g[2] == (nz + G.klen - 1) / G.klen && (!kch || G.klen == (nz + kch - 1) / kch), "W %d (%d, %d, %d) chunks %d: klen %d, %d chunks", W, nx, ny, nz, kch, G.klen, G.g[2]);
    if (!kch) CHECK(G.klen == (nz + god_chunks_slots(G.g[0] * G.g[1], nz, 512) - 1) / god_chunks_slots(G.g[0] * G.g[1], nz, 512), "W %d: the chunk rule", W);
    std::vector<int> kc(nz, 0);
    for (int bz = 0; bz < G.g[2]; bz++) {
      int k0, k1; god_planes(lo[2], hi[2], G.klen, bz, k0, k1);
      CHECK(k0 <= k1 && k0 >= lo[2] && k1 <= hi[2], "W %d: chunk %d is %d..%d", W, bz, k0, k1);
      for (int k = std::max(k0, lo[2]); k <= std::min(k1, hi[2]); k++) kc[k - lo[2]]++;
    }
    for (int k = 0; k < nz; k++) CHECK(kc[k] == 1, "W %d (%d, %d, %d) chunks %d: plane %d in %d chunks", W, nx, ny, nz, kch, k, kc[k]);
    if (kch) continue;
    std::vector<int> cov((size_t)nx * ny, 0);
    for (int by = 0; by < G.g[1]; by++) for (int bx = 0; bx < G.g[0]; bx++) {
      std::vector<int> slot((size_t)S.W * S.rows, 0);
      int f0[2] = { 1 << 30, 1 << 30 }, f1[2] = { -(1 << 30), -(1 << 30) }, w0[2] = { 1 << 30, 1 << 30 }, w1[2] = { -(1 << 30), -(1 << 30) };
      n_wg++;
      for (int ty = 0; ty < THY; ty++) for (int tx = 0; tx < 64; tx++) {
        int lane, row;
        const bool live = god_thread(W, tx, ty, lane, row, THY);
        CHECK(live && lane >= 0 && lane < S.W && row >= 0 && row < S.rows, "W %d thread (%d, %d): live %d lane %d row %d", W, tx, ty, live, lane, row);
        if (!(live && lane >= 0 && lane < S.W && row >= 0 && row < S.rows)) continue;
        slot[(size_t)row * S.W + lane]++;
        const GodCell C = god_cell(lo, hi, S, bx, by, lane, row, live);
        f0[0] = std::min(f0[0], C.i); f1[0] = std::max(f1[0], C.i); f0[1] = std::min(f0[1], C.j); f1[1] = std::max(f1[1], C.j);
        if (!C.own) continue;
        const bool in = C.i >= lo[0] && C.i <= hi[0] && C.j >= lo[1] && C.j <= hi[1];
        CHECK(in, "W %d wg (%d, %d) owns (%d, %d) outside the range", W, bx, by, C.i, C.j);
        if (in) cov[(size_t)(C.j - lo[1]) * nx + (C.i - lo[0])]++;
        w0[0] = std::min(w0[0], C.i); w1[0] = std::max(w1[0], C.i); w0[1] = std::min(w0[1], C.j); w1[1] = std::max(w1[1], C.j);
      }
      for (int q : slot) CHECK(q == 1, "W %d: a (lane, row) of the workgroup held by %d threads", W, q);
      CHECK(w0[0] <= w1[0], "W %d (%d, %d): workgroup (%d, %d) owns nothing", W, nx, ny, bx, by);
      for (int bz = 0; bz < G.g[2]; bz++) for (int upd = 0; upd < 2; upd++) {
        int a0[3], a1[3], k0, k1;
        god_footprint(lo, hi, S, G.klen, bx, by, bz, upd != 0, a0, a1);
        god_planes(lo[2], hi[2], G.klen, bz, k0, k1);
        CHECK(a0[0] == f0[0] && a1[0] == f1[0] && a0[1] == f0[1] && a1[1] == f1[1] && a0[2] == k0 - 2 && a1[2] == k1 + 2 + upd, "W %d wg (%d, %d, %d): footprint", W, bx, by, bz);
        // one cell around what the workgroup owns, and never below the range grown by one; above it only in a remainder tile
        CHECK(a0[0] == w0[0] - 1 && a0[1] == w0[1] - 1 && a0[0] >= lo[0] - 1 && a0[1] >= lo[1] - 1, "W %d wg (%d, %d): footprint starts at (%d, %d), owns from (%d, %d)", W, bx, by, a0[0], a0[1], w0[0], w0[1]);
        CHECK(a1[0] >= w1[0] + 1 && a1[1] >= w1[1] + 1, "W %d wg (%d, %d): footprint ends at (%d, %d), owns to (%d, %d)", W, bx, by, a1[0], a1[1], w1[0], w1[1]);
        CHECK((a1[0] <= hi[0] + 1 || bx == G.g[0] - 1) && (a1[1] <= hi[1] + 1 || by == G.g[1] - 1), "W %d wg (%d, %d): an inner tile leaves the grown range", W, bx, by);
        CHECK(a1[0] == w1[0] + 1 || w1[0] == hi[0], "W %d wg (%d, %d): x", W, bx, by);
        CHECK(a1[1] == w1[1] + 1 || w1[1] == hi[1], "W %d wg (%d, %d): y", W, bx, by);
      }
    }
    long bad = 0;
    for (int c : cov) bad += c != 1;
    CHECK(bad == 0, "W %d, range %d x %d: %ld cells of a plane not owned exactly once", W, nx, ny, bad);
  }
}

#define FORM(...) GOD_FORM_HALF(__VA_ARGS__),
static const std::vector<GodForm> MK_MH = { GOD_MK_MH_FORMS(FORM) };
static void check_forms() {
  CHECK(MK_MH.size() == 7, "kk_mk_F_mh: %zu forms", MK_MH.size());
  CHECK(!god_half_fits(128, 128, false, 128) && god_half_fits(128, 128, true, 128) && !god_half_fits(127, 300, true, 128) && !god_half_fits(300, 127, true, 128) && god_half_fits(1, 1, true, 1), "god_half_fits");
  // VDN_GOD_NARROW carries the half form: 1 (the default) wide boxes in 16 lanes, 16 / 32 every box in that width, anything else off
  for (int v = -2; v <= 40; v++) {
    const GodHalf H = god_half_switch(v);
    CHECK(H.on == (v == 1 || v == 16 || v == 32) && H.W == (v == 32 ? 32 : 16) && H.min == (v == 1 ? 128 : 1), "god_half_switch(%d): on %d min %d W %d", v, H.on, H.min, H.W);
    CHECK(god_half_fits(127, 127, H.on, H.min) == (v == 16 || v == 32) && god_half_fits(128, 128, H.on, H.min) == H.on, "god_half_switch(%d) with god_half_fits", v);
  }
  for (int m = 0; m < 512; m++) {
    const bool any = m & 1, inflow = m & 2, p2 = m & 4, upd = m & 8, cons = m & 16, minion = m & 32, cols = m & 128, batched = m & 256;
    const int sp = god_mk_sp(cons, minion, (m >> 6) & 1);
    const GodForm today = god_mk_form(any, inflow, p2, upd, sp, cols, batched);
    CHECK(!today.half && today == god_mk_form(any, inflow, p2, upd, sp, cols, batched, false), "inputs %d: the form without the half argument", m);
    const GodForm h = god_mk_form(any, inflow, p2, upd, sp, cols, batched, true);
    const bool admits = !batched && upd && p2 && any && !inflow;              // what a launch of kk_mk_F_mc needs of the form (the remainder column apart)
    if (!admits) { CHECK(h == today, "inputs %d: today's form cannot be the column grid's, yet the form changes", m); continue; }
    CHECK(h.half && !h.cols && std::find(MK_MH.begin(), MK_MH.end(), h) != MK_MH.end(), "inputs %d: half form (%d %d %d %d %d %d %d %d) has no instantiation", m, h.bc, h.inl, h.upd, h.pw2, h.sp, h.nar, h.cols, h.half);
    GodForm back = h; back.half = false; back.cols = today.cols;
    CHECK(back == today && today.cols == cols, "inputs %d: the half form differs from today's in more than cols and half", m);
  }
}

int main() {
  long ranges = 0;
  for (int W : { 16, 32 })
    for (int nx : { 1, 2, 13, 14, 15, 16, 28, 29, 30, 31, 33, 60, 61, 128, 129, 257, 300 }) for (int ny : { 1, 5, 6, 7, 14, 15, 16, 29, 70 }) for (int nz : { 1, 2, 6, 13, 40 }) { check_range(nx, ny, nz, W); ranges++; }
  check_forms();
  if (fails) { printf("%d checks failed\n", fails); return 1; }
  printf("OK %ld ranges, %ld workgroups walked, %zu instantiations in the list\n", ranges, n_wg, MK_MH.size());
  return 0;
}
