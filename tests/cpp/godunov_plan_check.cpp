// godunov_plan_check.cpp -- holds varden_amd/csrc/godunov_plan.h without a GPU.  Over a sweep of face ranges and, for each, the full-tile grid, the
// column grid where it applies and the batched grid in every segment width (0 and 6 .. 32), it walks every thread of every workgroup the way the
// marches do (god_thread, god_cell, god_planes, god_col, god_batch_wg) and checks that
//   * every (i, j, k) of the range is owned exactly once and nothing outside it is owned; the narrow column's workgroups that leave would own nothing.
//     Ownership is a product -- own(bx, by, thread) and k in k0(bz) .. k1(bz) -- so (i, j) and k are counted separately: each exactly once is the claim;
//   * the footprint the touch rule uses (god_footprint) equals the minimum and maximum over the workgroup's threads of the (i, j) they compute and
//     its planes k0 - 2 .. k1 + 2 (one more with the update);
//   * the touch rule is conservative: the marches apply a rule at lo[d] on a flagged low face, at hi[d] and hi[d] + 1 on a flagged high one (bcw and
//     Z_WORD of mk_F_m_body); no workgroup that does not touch has such a position in its footprint, for all 64 sets of flagged faces;
//   * the form choosers stay inside their family's instantiation list over the whole cross product of their inputs, and give the pinned form on every
//     branch of the six if / else ladders they replaced;
//   * the chunk lengths are the ones tests/test_godunov_phases_gpu.py expects on its shapes.
// "klen nx ny nz chunks ..." (groups of four; a face range and VDN_FUSED_KCHUNKS) prints per group the column grid's klen (-1: none) and the full-tile
// grid's: tests/test_godunov_plan_cpu.py compares them with the GPU test's Python mirror.  Built plain and under the address / undefined-behaviour
// sanitizers.  Prints "OK ..." and returns 0.
#include "godunov_plan.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (fails++ < 20) { printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Range { int lo[3], hi[3]; };
static long n_wg = 0;

// one workgroup (bx, by) of segments of W lanes over the range r: counts the cells its threads own into cov (a plane of `whole`), returns the extent of what they compute
static void walk_wg(const Range &whole, const Range &r, int W, int bx, int by, std::vector<int> &cov, int f0[2], int f1[2], bool leaves) {
  const GodSeg S = god_seg(W);
  const int nx = whole.hi[0] - whole.lo[0] + 1;
  std::vector<int> slot((size_t)S.W * S.rows, 0);
  f0[0] = f0[1] = 1 << 30; f1[0] = f1[1] = -(1 << 30);
  n_wg++;
  for (int ty = 0; ty < TNY; ty++) for (int tx = 0; tx < 64; tx++) {
    int lane, row;
    const bool live = god_thread(W, tx, ty, lane, row);
    CHECK(lane >= 0 && lane < S.W && row >= 0 && row < S.rows, "W %d thread (%d, %d): lane %d row %d", W, tx, ty, lane, row);
    if (live) slot[(size_t)row * S.W + lane]++;
    const GodCell C = god_cell(r.lo, r.hi, S, bx, by, lane, row, live);
    f0[0] = std::min(f0[0], C.i); f1[0] = std::max(f1[0], C.i); f0[1] = std::min(f0[1], C.j); f1[1] = std::max(f1[1], C.j);
    if (!C.own) continue;
    CHECK(!leaves, "W %d wg (%d, %d) leaves early but owns (%d, %d)", W, bx, by, C.i, C.j);
    const bool in = C.i >= r.lo[0] && C.i <= r.hi[0] && C.j >= r.lo[1] && C.j <= r.hi[1];
    CHECK(in, "W %d wg (%d, %d) owns (%d, %d) outside the range", W, bx, by, C.i, C.j);
    if (in) cov[(size_t)(C.j - whole.lo[1]) * nx + (C.i - whole.lo[0])]++;
  }
  for (int q : slot) CHECK(q == 1, "W %d: a (lane, row) of the workgroup held by %d live threads", W, q);
}
// footprint against the independent one, and the touch rule on it, for every k-chunk of the tile.  r: the range the workgroup marches (the column grid
// cuts it along x); whole: the face range of the box, whose faces carry the rules (the kernels test against F.lo / F.hi, the whole box)
static void check_touch(const Range &whole, const Range &r, int W, int klen, int gz, int bx, int by, const int f0[2], const int f1[2]) {
  int blo[3], bhi[3];                                     // the box of cells behind the face range
  for (int d = 0; d < 3; d++) { blo[d] = whole.lo[d]; bhi[d] = whole.hi[d] - 1; }
  for (int bz = 0; bz < gz; bz++) for (int upd = 0; upd < 2; upd++) {
    int a0[3], a1[3], k0, k1;
    god_footprint(r.lo, r.hi, god_seg(W), klen, bx, by, bz, upd != 0, a0, a1);
    god_planes(r.lo[2], r.hi[2], klen, bz, k0, k1);
    CHECK(a0[0] == f0[0] && a1[0] == f1[0] && a0[1] == f0[1] && a1[1] == f1[1] && a0[2] == k0 - 2 && a1[2] == k1 + 2 + upd,
          "W %d wg (%d, %d, %d): footprint (%d..%d, %d..%d, %d..%d), threads compute (%d..%d, %d..%d), planes %d..%d", W, bx, by, bz, a0[0], a1[0], a0[1], a1[1], a0[2], a1[2], f0[0], f1[0], f0[1], f1[1], k0, k1);
    for (int m = 0; m < 64; m++) {
      int mode[3][2];
      for (int d = 0; d < 3; d++) for (int sd = 0; sd < 2; sd++) mode[d][sd] = (m >> (2 * d + sd)) & 1 ? 1 + (m + d) % 4 : 0;
      if (god_touch(a0, a1, blo, bhi, [&](int d, int sd) { return mode[d][sd]; })) continue;
      for (int d = 0; d < 3; d++) {
        const bool lo_in = mode[d][0] && a0[d] <= blo[d] && blo[d] <= a1[d], hi_in = mode[d][1] && a0[d] <= bhi[d] + 1 && bhi[d] <= a1[d];
        CHECK(!lo_in && !hi_in, "W %d wg (%d, %d, %d) faces %d: untouched, yet direction %d of its footprint %d..%d holds a rule's position (box %d..%d)", W, bx, by, bz, m, d, a0[d], a1[d], blo[d], bhi[d]);
      }
    }
  }
}
static void check_planes(const Range &r, const GodGrid &G, const char *what) {
  const int nz = r.hi[2] - r.lo[2] + 1;
  std::vector<int> kc(nz, 0);
  CHECK(G.klen >= 1 && G.g[2] == (nz + G.klen - 1) / G.klen, "%s: klen %d, %d chunks for %d planes", what, G.klen, G.g[2], nz);
  for (int bz = 0; bz < G.g[2]; bz++) {
    int k0, k1; god_planes(r.lo[2], r.hi[2], G.klen, bz, k0, k1);
    CHECK(k0 <= k1 && k0 >= r.lo[2] && k1 <= r.hi[2], "%s: chunk %d is %d..%d", what, bz, k0, k1);
    for (int k = std::max(k0, r.lo[2]); k <= std::min(k1, r.hi[2]); k++) kc[k - r.lo[2]]++;
  }
  for (int k = 0; k < nz; k++) CHECK(kc[k] == 1, "%s: plane %d in %d chunks", what, k, kc[k]);
}
static void check_cover(const Range &r, const std::vector<int> &cov, const char *what, int W) {
  long bad = 0;
  for (int c : cov) bad += c != 1;
  CHECK(bad == 0, "%s W %d, range %d x %d: %ld cells of a plane not owned exactly once", what, W, r.hi[0] - r.lo[0] + 1, r.hi[1] - r.lo[1] + 1, bad);
}
static long check_range(int nx, int ny, int nz) {
  Range r; const int lo[3] = { 3, -5, 7 }, n[3] = { nx, ny, nz };
  for (int d = 0; d < 3; d++) { r.lo[d] = lo[d]; r.hi[d] = lo[d] + n[d] - 1; }
  int f0[2], f1[2];
  // full tiles, with the chunk rule and with a forced chunk count
  for (int kch : { 0, 1, 5, 16 }) {
    const GodGrid G = god_grid_tiles(nx, ny, nz, kch);
    check_planes(r, G, "tiles");
    if (kch) continue;
    std::vector<int> cov((size_t)nx * ny, 0);
    for (int by = 0; by < G.g[1]; by++) for (int bx = 0; bx < G.g[0]; bx++) { walk_wg(r, r, 64, bx, by, cov, f0, f1, false); check_touch(r, r, 64, G.klen, G.g[2], bx, by, f0, f1); }
    check_cover(r, cov, "tiles", 64);
  }
  // full tile columns + the narrow remainder column
  GodGrid M;
  CHECK(!god_grid_cols(nx, ny, nz, false, M), "column grid with the switch off");
  if (god_grid_cols(nx, ny, nz, true, M)) {
    CHECK(M.full >= 1 && M.g[0] == M.full + 1 && M.segw == nx - M.full * FNX + 2 && M.segw <= 32, "cols: full %d segw %d", M.full, M.segw);
    check_planes(r, M, "cols");
    std::vector<int> cov((size_t)nx * ny, 0);
    for (int by = 0; by < M.g[1]; by++) for (int bx = 0; bx < M.g[0]; bx++) {
      const GodCol C = god_col(r.lo, r.hi, M.full, M.segw, bx, by);
      Range rr = r; rr.lo[0] = C.lo0; rr.hi[0] = C.hi0;
      CHECK(C.narrow == (bx == M.full) && (C.narrow || !C.leave) && C.W == (C.narrow ? M.segw : 64), "cols: wg (%d, %d)", bx, by);
      walk_wg(r, rr, C.W, C.bx, by, cov, f0, f1, C.leave);
      if (!C.leave) check_touch(r, rr, C.W, M.klen, M.g[2], C.bx, by, f0, f1);
    }
    check_cover(r, cov, "cols", M.segw);
  }
  // the batched grid: every width, through the linear workgroup index; the search takes the width with the fewest workgroups
  const GodGrid S0 = god_grid_small(nx, ny, nz, false), S1 = god_grid_small(nx, ny, nz, true);
  CHECK(S0.segw == 0 && S0.klen == S1.klen && S0.g[2] == S1.g[2], "small: switch off");
  check_planes(r, S1, "small");
  int fewest = S0.g[0] * S0.g[1];
  for (int W = 0; W <= 32; W = W ? W + 1 : 6) {
    const GodSeg S = god_seg(W ? W : 64);
    const int g[3] = { (nx + S.ownx - 1) / S.ownx, (ny + S.owny - 1) / S.owny, S1.g[2] };
    fewest = std::min(fewest, g[0] * g[1]);
    if (W == S1.segw) CHECK(g[0] == S1.g[0] && g[1] == S1.g[1], "small: grid of the chosen width %d", W);
    std::vector<int> cov((size_t)nx * ny, 0);
    for (int l = 0; l < g[0] * g[1] * g[2]; l++) {
      int bx, by, bz; god_batch_wg(g[0], g[1], l, bx, by, bz);
      CHECK(bx >= 0 && bx < g[0] && by >= 0 && by < g[1] && bz >= 0 && bz < g[2] && l == (bz * g[1] + by) * g[0] + bx, "small: workgroup %d", l);
      if (bz) continue;                                   // the planes are check_planes': one sweep of the tiles
      walk_wg(r, r, S.W, bx, by, cov, f0, f1, false); check_touch(r, r, S.W, S1.klen, g[2], bx, by, f0, f1);
    }
    check_cover(r, cov, "small", W);
  }
  CHECK(S1.g[0] * S1.g[1] == fewest, "small: width %d takes %d workgroups per chunk, the fewest is %d", S1.segw, S1.g[0] * S1.g[1], fewest);
  return 1;
}

// ---- forms ----------------------------------------------------------------------------------------------------------------------------------
#define FORM(...) GOD_FORM(__VA_ARGS__),
static const std::vector<GodForm> MK_M = { GOD_MK_M_FORMS(FORM) }, MK_MC = { GOD_MK_MC_FORMS(FORM) }, MK_MB = { GOD_MK_MB_FORMS(FORM) };
static const std::vector<GodForm> VP_M = { GOD_VP_M_FORMS(FORM) }, VP_MC = { GOD_VP_MC_FORMS(FORM) }, VP_MB = { GOD_VP_MB_FORMS(FORM) };
static bool in_list(const GodForm &f, const std::vector<GodForm> &L) { return std::find(L.begin(), L.end(), f) != L.end(); }
static void check_list(const std::vector<GodForm> &L, size_t n, const char *name) {
  CHECK(L.size() == n, "%s: %zu forms, %zu instantiations expected", name, L.size(), n);
  for (size_t a = 0; a < L.size(); a++) for (size_t b = a + 1; b < L.size(); b++) CHECK(!(L[a] == L[b]), "%s: form %zu listed twice", name, a);
}
static void check_forms() {
  check_list(MK_M, 22, "kk_mk_F_m"); check_list(MK_MC, 7, "kk_mk_F_mc"); check_list(MK_MB, 6, "kk_mk_F_mb");
  check_list(VP_M, 7, "kk_vp_F_m"); check_list(VP_MC, 2, "kk_vp_F_mc"); check_list(VP_MB, 10, "kk_vp_F_mb");
  CHECK(god_mk_sp(true, false, 1) == SP_RT && god_mk_sp(true, true, 1) == SP_RT && god_mk_sp(true, true, 0) == (SP_CONS | SP_MINION) && god_mk_sp(false, true, 1) == (SP_FMODE1 | SP_MINION), "god_mk_sp");
  for (int m = 0; m < 512; m++) {
    const bool any = m & 1, inflow = m & 2, p2 = m & 4, upd = m & 8, cons = m & 16, minion = m & 32, cols = m & 128, batched = m & 256;
    const int fmode = (m >> 6) & 1;
    GodForm f = god_mk_form(any, inflow, p2, upd, god_mk_sp(cons, minion, fmode), cols, batched);
    for (int nar = 0; nar < (batched ? 2 : 1); nar++) {
      f.nar = nar != 0;
      CHECK(in_list(f, batched ? MK_MB : f.cols ? MK_MC : MK_M), "mkflux inputs %d: form (%d %d %d %d %d %d %d) has no instantiation", m, f.bc, f.inl, f.upd, f.pw2, f.sp, f.nar, f.cols);
    }
    f = god_vp_form(any, inflow, p2, minion, cols, batched);
    for (int nar = 0; nar < (batched ? 2 : 1); nar++) {
      f.nar = nar != 0;
      CHECK(in_list(f, batched ? VP_MB : f.cols ? VP_MC : VP_M), "velpred inputs %d: form (%d %d %d %d %d %d %d) has no instantiation", m, f.bc, f.inl, f.upd, f.pw2, f.sp, f.nar, f.cols);
    }
  }
  // one row per branch of the ladders these choosers replaced (written from the ladders): inputs any, inflow, p2, upd, cols, batched -> form.
  // sp / minion is swept inside: S marks the rows whose form carries it, the others are SP_RT
  const int S = 99, RT = SP_RT;
  const struct { bool mk, any, inflow, p2, upd, cols, batched; GodForm f; } rows[] = {
    // mkflux, one box, the update rides along
    { true, false, false, true, true, true, false, { false, false, true, true, S, false, false } },      // no face: never the column grid
    { true, false, false, false, true, true, false, { false, false, true, false, RT, false, false } },
    { true, true, true, true, true, true, false, { true, true, true, false, RT, false, false } },         // inflow keeps the division
    { true, true, true, false, true, false, false, { true, true, true, false, RT, false, false } },
    { true, true, false, true, true, true, false, { true, false, true, true, S, false, true } },          // kk_mk_F_mc
    { true, true, false, true, true, false, false, { true, false, true, true, S, false, false } },
    { true, true, false, false, true, true, false, { true, false, true, false, RT, false, false } },
    // mkflux, one box, edge states and fluxes stored
    { true, false, false, true, false, true, false, { false, false, false, true, RT, false, false } },
    { true, false, false, false, false, true, false, { false, false, false, false, RT, false, false } },
    { true, true, true, true, false, true, false, { true, true, false, false, RT, false, false } },
    { true, true, false, true, false, true, false, { true, false, false, true, RT, false, false } },
    { true, true, false, false, false, true, false, { true, false, false, false, RT, false, false } },
    // mkflux, batched (wide and narrow launch alike): no bc = 0 form
    { true, true, true, true, true, true, true, { true, true, false, false, RT, false, false } },
    { true, false, false, true, false, false, true, { true, false, false, true, RT, false, false } },
    { true, false, false, false, false, false, true, { true, false, false, false, RT, false, false } },
    // velpred, batched
    { false, false, false, true, false, true, true, { false, false, false, true, RT, false, false } },
    { false, false, false, false, false, true, true, { false, false, false, false, RT, false, false } },
    { false, true, true, true, false, true, true, { true, true, false, false, RT, false, false } },
    { false, true, false, true, false, true, true, { true, false, false, true, RT, false, false } },
    { false, true, false, false, false, true, true, { true, false, false, false, RT, false, false } },
    // velpred, one box (sp: use_minion compiled in, SP_MINION or 0)
    { false, false, false, true, false, true, false, { false, false, false, true, S, false, false } },
    { false, false, false, false, false, true, false, { false, false, false, false, RT, false, false } },
    { false, true, true, true, false, true, false, { true, true, false, false, RT, false, false } },
    { false, true, false, true, false, true, false, { true, false, false, true, S, false, true } },       // kk_vp_F_mc
    { false, true, false, true, false, false, false, { true, false, false, true, S, false, false } },
    { false, true, false, false, false, true, false, { true, false, false, false, RT, false, false } },
  };
  int row = 0;
  for (const auto &q : rows) {
    for (int sp : { 0, SP_CONS, SP_MINION, SP_CONS | SP_MINION, SP_FMODE1, SP_FMODE1 | SP_MINION, SP_RT }) {
      GodForm want = q.f;
      const bool minion = sp != SP_RT && (sp & SP_MINION);
      if (want.sp == S) want.sp = q.mk ? sp : (minion ? SP_MINION : 0);
      const GodForm got = q.mk ? god_mk_form(q.any, q.inflow, q.p2, q.upd, sp, q.cols, q.batched) : god_vp_form(q.any, q.inflow, q.p2, minion, q.cols, q.batched);
      CHECK(got == want, "ladder row %d, sp %d: form (%d %d %d %d %d %d %d), the ladder gave (%d %d %d %d %d %d %d)", row, sp, got.bc, got.inl, got.upd, got.pw2, got.sp, got.nar, got.cols,
            want.bc, want.inl, want.upd, want.pw2, want.sp, want.nar, want.cols);
    }
    row++;
  }
  CHECK(!god_use_batched(0, 0, true) && god_use_batched(1, 8, true) && !god_use_batched(1, 8, false) && god_use_batched(2, 2L * 95 * 96 * 96, false) && !god_use_batched(16, 16L * 96 * 96 * 96, false)
        && god_use_batched(17, 17L * 96 * 96 * 96, false), "god_use_batched");
}

// ---- the chunk lengths tests/test_godunov_phases_gpu.py expects (its shapes are boxes: one face more per direction) ---------------------------------
static int klen_cols(int nx, int ny, int nz) { GodGrid M; return god_grid_cols(nx, ny, nz, true, M) ? M.klen : -1; }
static void check_klens() {
  const int want[5] = { 1, 2, 3, 4, 6 }, col_z[5] = { 15, 19, 34, 49, 82 }, step_z[5] = { 12, 24, 40, 56, 88 };
  for (int q = 0; q < 5; q++) {
    CHECK(klen_cols(73, 15, col_z[q] + 1) == want[q], "COL_SHAPES (72, 14, %d): klen %d, expected %d", col_z[q], klen_cols(73, 15, col_z[q] + 1), want[q]);
    CHECK(klen_cols(73, 17, step_z[q] + 1) == want[q], "STEP_SHAPES (72, 16, %d): klen %d, expected %d", step_z[q], klen_cols(73, 17, step_z[q] + 1), want[q]);
  }
  CHECK(klen_cols(25, 15, 13) == -1 && klen_cols(25, 17, 13) == -1, "NARROW_SHAPE and (24, 16, 12) have no column grid");
  const int klen[5] = { 1, 2, 3, 4, 7 }, ch[5] = { 13, 7, 5, 4, 2 };
  for (int q = 0; q < 5; q++) CHECK(god_grid_tiles(25, 15, 13, ch[q]).klen == klen[q], "NARROW_SHAPE, %d chunks: klen %d, expected %d", ch[q], god_grid_tiles(25, 15, 13, ch[q]).klen, klen[q]);
}

int main(int argc, char **argv) {
  if (argc >= 2 && !strcmp(argv[1], "klen")) {
    for (int a = 2; a + 3 < argc; a += 4) {
      const int nx = atoi(argv[a]), ny = atoi(argv[a + 1]), nz = atoi(argv[a + 2]), ch = atoi(argv[a + 3]);
      printf("%d %d\n", klen_cols(nx, ny, nz), god_grid_tiles(nx, ny, nz, ch).klen);
    }
    return 0;
  }
  long ranges = 0;
  for (int nx : { 1, 5, 8, 30, 31, 61, 62, 63, 72, 92, 93, 124, 125, 257 }) for (int ny : { 1, 6, 7, 15, 47 }) for (int nz : { 1, 2, 13, 49, 97 }) ranges += check_range(nx, ny, nz);
  check_forms();
  check_klens();
  if (fails) { printf("%d checks failed\n", fails); return 1; }
  printf("OK %ld ranges, %ld workgroups walked, %zu + %zu instantiations in the lists\n", ranges, n_wg, MK_M.size() + MK_MC.size() + MK_MB.size(), VP_M.size() + VP_MC.size() + VP_MB.size());
  return 0;
}
