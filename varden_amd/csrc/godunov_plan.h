// godunov_plan.h -- the tiling and the launch forms of the fused Godunov marches (kk_mk_F_* and kk_vp_F_* in godunov.hip): the tile constants, the
// k-chunk rule, the four grids built on it, which thread of which workgroup computes and owns which cell, a workgroup's footprint and the rule that
// decides from it whether the workgroup needs the boundary code, the template instantiation a launch takes, and when a level is batched.  Integers and
// plain structs only: no HIP runtime, no ctx(), no sw() -- what a switch decides arrives as an argument.  The kernels and the launchers read it, and so
// does tests/cpp/godunov_plan_check.cpp with a host compiler, so the mapping exists in one place.
//
// A workgroup is 64 x TNY threads (64 x THY in the half form, god_grid_half) and marches its tile through k0 .. k1 of the face range r.  Its rows are cut into segments of W lanes (W = 64: one
// row per wave, the full-width tile; W < 64: 64 / W rows per wave): the first and last lane of a segment and the first and last row of a workgroup only
// feed their neighbours, so tiles overlap by two cells.  The workgroup index (bx, by, bz) is the one after the XCD-aware remap (a bijection of the grid).
#pragma once
#if defined(__HIPCC__)
#define GOD_FN __host__ __device__ __forceinline__
#define GOD_UNROLL _Pragma("unroll")
#define GOD_MIN(a, b) min(a, b)
#else
#define GOD_FN inline
#define GOD_UNROLL
#define GOD_MIN(a, b) ((a) < (b) ? (a) : (b))
#endif

constexpr int TNY = 8;                      // rows per tile: workgroup = 64 x TNY threads
constexpr int THY = 4;                      // the half workgroup (kk_mk_F_mh): 64 x THY threads, two of them per compute unit
constexpr int FNX = 62, FNY = TNY - 2;      // cells a full-width tile owns per row / rows it owns
// SP: the launch-uniform flags of a one-box march as a template argument -- cons, use_minion and (UPD) the update's forcing mode compiled in, so that
// neither arm of a flag nor the copies around it stay in the plane loop (f_bases, tvq, the stage-D chains, the update); SP_RT: read from FArgs at run
// time (the box-batched launches, whose descriptors differ in them, and the rarely taken forms).  vp_F_m_body: use_minion only.
constexpr int SP_RT = -1, SP_CONS = 1, SP_MINION = 2, SP_FMODE1 = 4;

// ---- the map as text ------------------------------------------------------------------------------------------------------------------------
// The one-box marches hold 220 to 251 of 256 VGPRs, and what the register allocator makes of them depends on the exact shape of the code in front of
// the plane loop: the expressions below as inline functions moved up to 20 of the 54 instantiations by 1 to 6 VGPRs, and one arrangement sent four of
// them into scratch.  So the pieces a kernel expands in place are macros, the text the kernels always had -- their machine code is the parent's,
// instruction for instruction -- and the functions of the next section, which the host and the check call, are the same macros expanded: one text.
// thread (tx, ty) of a workgroup in segments of W lanes: the rows the workgroup carries, the thread's lane in its segment and its row; live = false: a
// lane left over after the wave's last segment (it owns nothing and rides along in the last row)
// (TY: the waves of the workgroup, TNY or THY)
#define GOD_THREAD_T(TY, W, tx, ty, rows, live, lane, row)                                                                               \
  const int rpw_ = 64 / (W), seg_ = (tx) / (W);                                                                                          \
  rows = (TY) * rpw_; live = seg_ < rpw_; lane = (tx) - seg_ * (W);                                                                      \
  row = live ? (ty) * rpw_ + seg_ : rows - 1;
#define GOD_THREAD(W, tx, ty, rows, live, lane, row) GOD_THREAD_T(TNY, W, tx, ty, rows, live, lane, row)
// the cell (i, j) that lane / row of workgroup (bx, by) computes in the range lo .. hi, and whether it owns it (ownx, owny: GodSeg)
#define GOD_CELL(lo, hi, ownx, owny, bx, by, lane, row, live, i, j, own)                                                                 \
  const int i = (lo)[0] - 1 + (bx) * (ownx) + (lane), j = (lo)[1] - 1 + (by) * (owny) + (row);                                           \
  const bool own = (live) && (lane) >= 1 && (lane) <= (ownx) && (row) >= 1 && (row) <= (owny) && i <= (hi)[0] && j <= (hi)[1];
// the planes k0 .. k1 of k-chunk bz; workgroup l of a box's gx x gy x g[2] in a batched launch (gy: g[1], at least 1)
#define GOD_PLANES(lo2, hi2, klen, bz, k0, k1) const int k0 = (lo2) + (bz) * (klen), k1 = GOD_MIN(k0 + (klen) - 1, hi2);
#define GOD_BATCH_WG(gx, gy, l, BX, BY, BZ) const int BX = (l) % (gx), BY = ((l) / (gx)) % (gy), BZ = (l) / ((gx) * (gy));
// everything workgroup (bx, by, bz) of tw lanes x th rows (ownx = tw - 2 columns its own) computes lies in a0 .. a1: its lanes and rows, and its planes with the two a march runs
// ahead and behind (one more with the update, upd: the lower z-face of its successor's first plane)
#define GOD_FOOTPRINT(lo, hi, tw, th, ownx, klen, upd, bx, by, bz, a0, a1)                                                               \
  const int i0_ = (lo)[0] - 1 + (bx) * (ownx), i1_ = i0_ + (tw) - 1, j0_ = (lo)[1] - 1 + (by) * ((th) - 2), j1_ = j0_ + (th) - 1;    \
  const int k0_ = (lo)[2] + (bz) * (klen) - 2, k1_ = GOD_MIN((lo)[2] + (bz) * (klen) + (klen) - 1, (hi)[2]) + 2 + ((upd) ? 1 : 0);       \
  const int a0[3] = { i0_, j0_, k0_ }, a1[3] = { i1_, j1_, k1_ };
// touch = true when the footprint comes near a face of the box blo .. bhi (cells) that carries a rule (M0, M1: bc_mode of the low / high face of
// direction d, 0: none).  The marches apply rules at blo[d] on a low face, at bhi[d] and bhi[d] + 1 on a high one: a workgroup that does not touch runs
// the body without the boundary code.
#define GOD_TOUCH(touch, a0, a1, blo, bhi, d, M0, M1)                                                                                    \
  GOD_UNROLL                                                                                                                             \
  for (int d = 0; d < 3; d++) {                                                                                                          \
    if ((M0) && a0[d] <= (blo)[d] + 1) touch = true;                                                                                     \
    if ((M1) && a1[d] >= (bhi)[d] - 1) touch = true;                                                                                     \
  }

// the column grid (god_grid_cols): tile column bx == full is the remainder column, in segments of segw lanes over the range's last columns (lo0 .. hi0,
// counted from bx = 0) -- it needs fewer workgroups along y than the grid has, the others LEAVE at once; the columns before it are full-width tiles over
// the range cut short.  NO KERNEL EXPANDS THIS ONE: kk_mk_F_mc and kk_vp_F_mc restate it in their own text (with the macro kk_vp_F_mc takes two VGPRs
// more and the kk_mk_F_mc instantiations up to 7 % more instructions), so the column map exists three times -- here, for god_col and the check, and in the
// two kernels -- and only the bit-for-bit GPU tests (tests/test_godunov_phases_gpu.py) hold the kernels' copies against this one.  Change them together.
#define GOD_COL(lo, hi, full, segw, bx, by, narrow, tw, th, lo0, hi0, LEAVE)                                                             \
  const bool narrow = (bx) == (full);                                                                                                    \
  int tw = 64, th = TNY, lo0 = (lo)[0], hi0 = (hi)[0];                                                                                   \
  if (narrow) {                                                                                                                          \
    tw = (segw); th = TNY * (64 / (segw));                                                                                               \
    lo0 = (lo)[0] + (full) * FNX;                                                                                                        \
    if ((by) * (th - 2) > (hi)[1] - (lo)[1]) LEAVE;                                                                                      \
    bx = 0;                                                                                                                              \
  } else hi0 = (lo)[0] + (full) * FNX - 1;

// ---- segments, threads, cells, footprints ---------------------------------------------------------------------------------------------------------
struct GodSeg { int W, rows, ownx, owny; };         // lanes of a row segment, rows a workgroup carries, columns / rows it owns
GOD_FN GodSeg god_seg(int W, int TY = TNY) { return GodSeg{ W, TY * (64 / W), W - 2, TY * (64 / W) - 2 }; }
GOD_FN bool god_thread(int W, int tx, int ty, int &lane, int &row, int TY = TNY) {
  int rows; bool live;
  GOD_THREAD_T(TY, W, tx, ty, rows, live, lane, row)
  return live;
}
struct GodCell { int i, j; bool own; };             // the cell a thread computes, and whether it stores it
GOD_FN GodCell god_cell(const int lo[3], const int hi[3], const GodSeg &S, int bx, int by, int lane, int row, bool live) {
  GOD_CELL(lo, hi, S.ownx, S.owny, bx, by, lane, row, live, i, j, own)
  return GodCell{ i, j, own };
}
GOD_FN void god_planes(int lo2, int hi2, int klen, int bz, int &o0, int &o1) { GOD_PLANES(lo2, hi2, klen, bz, k0, k1) o0 = k0; o1 = k1; }
struct GodCol { bool narrow, leave; int W, bx, lo0, hi0; };
GOD_FN GodCol god_col(const int lo[3], const int hi[3], int full, int segw, int bx, int by) {
  bool leave = false;
  GOD_COL(lo, hi, full, segw, bx, by, narrow, tw, th, lo0, hi0, leave = true)
  return GodCol{ narrow, leave, tw, bx, lo0, hi0 };
}
GOD_FN void god_batch_wg(int gx, int gy, int l, int &bx, int &by, int &bz) { GOD_BATCH_WG(gx, gy, l, BX, BY, BZ) bx = BX; by = BY; bz = BZ; }
GOD_FN void god_footprint(const int lo[3], const int hi[3], const GodSeg &S, int klen, int bx, int by, int bz, bool upd, int o0[3], int o1[3]) {
  GOD_FOOTPRINT(lo, hi, S.W, S.rows, S.ownx, klen, upd, bx, by, bz, a0, a1)
  for (int d = 0; d < 3; d++) { o0[d] = a0[d]; o1[d] = a1[d]; }
}
template <class Mode> GOD_FN bool god_touch(const int a0[3], const int a1[3], const int blo[3], const int bhi[3], Mode mode) {      // mode(d, side)
  bool touch = false;
  GOD_TOUCH(touch, a0, a1, blo, bhi, d, mode(d, 0), mode(d, 1))
  return touch;
}

// ---- k-chunks and grids -------------------------------------------------------------------------------------------------------------------------
// one 512-thread workgroup per CU at a time: the chunk count (at most 16) is the one that fills the last round of workgroups best -- least rounds of 256
// workgroups x iterations per workgroup (a chunk's planes + 4)
GOD_FN int god_chunks(int tiles, int nz) {
  int best = 1; long long best_cost = -1;
  for (int ch = 1; ch <= 16 && ch <= nz; ch++) {
    const int kl = (nz + ch - 1) / ch, nch = (nz + kl - 1) / kl;
    const long long cost = (((long long)tiles * nch + 255) / 256) * (kl + 4);
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = ch; }
  }
  return best;
}
// two 256-thread workgroups per CU at a time (kk_mk_F_mh) are 512 workgroup slots: god_chunks' rule with the slot count as an argument
GOD_FN int god_chunks_slots(int tiles, int nz, int slots) {
  int best = 1; long long best_cost = -1;
  for (int ch = 1; ch <= 16 && ch <= nz; ch++) {
    const int kl = (nz + ch - 1) / ch, nch = (nz + kl - 1) / kl;
    const long long cost = (((long long)tiles * nch + slots - 1) / slots) * (kl + 4);
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = ch; }
  }
  return best;
}
// g: workgroups per direction; klen: planes per k-chunk; segw: lanes of the narrow segments (0: full-width tiles only); full: the full tile columns in
// front of the remainder column (column grid only)
struct GodGrid { int g[3], klen, segw, full; };
// full-width tiles over an nx x ny x nz range; kchunks: VDN_FUSED_KCHUNKS (0: god_chunks)
GOD_FN GodGrid god_grid_tiles(int nx, int ny, int nz, int kchunks) {
  GodGrid G; G.segw = 0; G.g[0] = G.full = (nx + FNX - 1) / FNX; G.g[1] = (ny + FNY - 1) / FNY;
  const int chunks = kchunks ? kchunks : god_chunks(G.g[0] * G.g[1], nz);
  G.klen = (nz + chunks - 1) / chunks; if (G.klen < 1) G.klen = 1;
  G.g[2] = (nz + G.klen - 1) / G.klen;
  return G;
}
// full 62-cell tile columns + one column of narrow segments for the remainder (kk_mk_F_mc, kk_vp_F_mc); false when the box has no remainder column worth
// it (narrow: VDN_GOD_NARROW).  The chunk count is chosen for the workgroups that do work.
GOD_FN bool god_grid_cols(int nx, int ny, int nz, bool narrow, GodGrid &G) {
  G.full = nx / FNX;
  const int rem = nx - G.full * FNX;
  if (!narrow || G.full < 1 || rem <= 0 || rem + 2 > 32) return false;
  G.segw = rem + 2;
  const int owny = god_seg(G.segw).owny, chunks = god_chunks(G.full * ((ny + FNY - 1) / FNY) + (ny + owny - 1) / owny, nz);
  G.klen = (nz + chunks - 1) / chunks;
  G.g[0] = G.full + 1; G.g[1] = (ny + FNY - 1) / FNY; G.g[2] = (nz + G.klen - 1) / G.klen;
  return true;
}
// half workgroups (kk_mk_F_mh) over an nx x ny x nz range: every tile in segments of W lanes (16 or 32: no lane of a wave is left over), THY * 64 / W rows,
// so a tile owns (W - 2) x (4 * 64 / W - 2) cells; kchunks: VDN_FUSED_KCHUNKS (0: god_chunks_slots over the 512 slots of two workgroups per CU)
GOD_FN GodGrid god_grid_half(int nx, int ny, int nz, int W, int kchunks) {
  const GodSeg S = god_seg(W, THY);
  GodGrid G; G.segw = W; G.full = 0; G.g[0] = (nx + S.ownx - 1) / S.ownx; G.g[1] = (ny + S.owny - 1) / S.owny;
  const int chunks = kchunks ? kchunks : god_chunks_slots(G.g[0] * G.g[1], nz, 512);
  G.klen = (nz + chunks - 1) / chunks; if (G.klen < 1) G.klen = 1;
  G.g[2] = (nz + G.klen - 1) / G.klen;
  return G;
}
// what VDN_GOD_NARROW = v says about the half form (the list of vdn_switches.h keeps its length, so the entry carries it): on for the default 1 (boxes
// whose face range is at least 128 wide in x and y, 16-lane segments) and for 16 / 32 (segments of that many lanes, boxes of any width: the tests);
// 0, 2 and anything else: off.  Whether the remainder column runs in narrow segments is v != 0, as before.
struct GodHalf { bool on; int min, W; };
GOD_FN GodHalf god_half_switch(int v) { return GodHalf{ v == 1 || v == 16 || v == 32, v == 1 ? 128 : 1, v == 32 ? 32 : 16 }; }
// the half form pays on wide boxes only (on, min: god_half_switch; min: the least width of the face range in x and y)
GOD_FN bool god_half_fits(int nx, int ny, bool on, int min) { return on && nx >= min && ny >= min; }
// a box of a batched launch: the boxes of a level fill the device together, so a box is cut along k only when it is tall; segments of the width that
// takes the fewest workgroups (segs: VDN_GOD_SEGW; 0: full-width tiles for every box)
GOD_FN GodGrid god_grid_small(int nx, int ny, int nz, bool segs) {
  GodGrid G; G.segw = 0;
  const int chunks = (nz + 47) / 48 > 1 ? (nz + 47) / 48 : 1;
  G.klen = (nz + chunks - 1) / chunks;
  G.g[0] = G.full = (nx + FNX - 1) / FNX; G.g[1] = (ny + FNY - 1) / FNY; G.g[2] = (nz + G.klen - 1) / G.klen;
  int best = G.g[0] * G.g[1];
  for (int w = 6; segs && w <= 32; w++) {
    const GodSeg S = god_seg(w);
    const int gx = (nx + S.ownx - 1) / S.ownx, gy = (ny + S.owny - 1) / S.owny;
    if (gx * gy < best) { best = gx * gy; G.segw = w; G.g[0] = gx; G.g[1] = gy; }
  }
  return G;
}
// one launch per stage for all boxes of a level (descriptors) or one set of launches per box (arguments by value)?  A level of an adaptive hierarchy
// (hundreds of 16^3 .. 32^3 boxes) is launch-bound box by box; a level of a few large boxes -- 512^3 cut into eight 256^3 boxes -- runs faster box by
// box: the by-value kernels need fewer registers (measured, eight 256^3 boxes on one GPU: scalar 52 -> 42 ms, velocity 76 -> 54 ms per step), and so does
// a level of one box (256^3: scalar 6.6 vs 5.6 ms, velocity 10.0 vs 8.2 ms).  force: VDN_GODUNOV_BATCH=1, the descriptors also for one box.
GOD_FN bool god_use_batched(int nboxes, long cells, bool force) {
  if (nboxes == 0) return false;
  if (force) return true;
  if (nboxes == 1) return false;
  return !(nboxes <= 16 && cells / nboxes >= 96L * 96 * 96);
}

// ---- launch forms -------------------------------------------------------------------------------------------------------------------------------
// the template arguments of a launch: bc: boundary code; inl: an inflow face (the ghost-value reads); upd: the update rides along (mkflux); pw2: every dx a
// power of two, divisions by dx as multiplications; sp: the compiled-in flags or SP_RT; nar: narrow segments (batched); cols: the column grid (_mc);
// half: half workgroups (_mh)
struct GodForm { bool bc, inl, upd, pw2; int sp; bool nar, cols, half; };
#define GOD_FORM(bc, inl, upd, pw2, sp, nar, cols) (GodForm{ (bc) != 0, (inl) != 0, (upd) != 0, (pw2) != 0, (sp), (nar) != 0, (cols) != 0, false })
#define GOD_FORM_HALF(bc, inl, upd, pw2, sp, nar, cols) (GodForm{ (bc) != 0, (inl) != 0, (upd) != 0, (pw2) != 0, (sp), (nar) != 0, (cols) != 0, true })
GOD_FN bool operator==(const GodForm &a, const GodForm &b) { return a.bc == b.bc && a.inl == b.inl && a.upd == b.upd && a.pw2 == b.pw2 && a.sp == b.sp && a.nar == b.nar && a.cols == b.cols && a.half == b.half; }
// The update-carrying power-of-two marches of a one-box level (what a step on 2^n cells runs) with the launch's flags compiled in: the combinations
// that occur -- a conservative or a convective scalar with the force of the call, a velocity component with the forcing term formed in place, each
// with and without use_minion; anything else takes the run-time form.
GOD_FN int god_mk_sp(bool cons, bool minion, int fmode) {
  if (cons && fmode) return SP_RT;
  return (cons ? SP_CONS : 0) | (minion ? SP_MINION : 0) | (fmode == 1 ? SP_FMODE1 : 0);
}
// The instantiations that exist, X(bc, inl, upd, pw2, sp, nar, cols), per kernel family; a form outside its family's list cannot be launched.
//   * the inflow forms keep the division (pw2 = 0): fewer instantiations;
//   * sp is compiled in only where pw2 is, and in kk_mk_F_m / _mc only with the update; the update forms with run-time flags stay unpeeled (peeled, the
//     inflow one needs scratch -- profiles/godunov_phases_ab.txt);
//   * the column grid exists for launches with boundary code only, so a box without a physical face keeps full tiles;
//   * the half workgroups exist where the column grid does (launches with boundary code and the update, sp compiled in or SP_RT) and take its place;
//   * the batched mkflux march has no bc = 0 form (its workgroups choose the lean body themselves: god_touch), the batched marches no sp and no update.
#define GOD_MK_SP_FORMS(X, bc, cols) X(bc, 0, 1, 1, 0, 0, cols) X(bc, 0, 1, 1, SP_CONS, 0, cols) X(bc, 0, 1, 1, SP_MINION, 0, cols) X(bc, 0, 1, 1, SP_CONS | SP_MINION, 0, cols) \
  X(bc, 0, 1, 1, SP_FMODE1, 0, cols) X(bc, 0, 1, 1, SP_FMODE1 | SP_MINION, 0, cols) X(bc, 0, 1, 1, SP_RT, 0, cols)
#define GOD_MK_M_FORMS(X) GOD_MK_SP_FORMS(X, 0, 0) GOD_MK_SP_FORMS(X, 1, 0) X(0, 0, 1, 0, SP_RT, 0, 0) X(1, 1, 1, 0, SP_RT, 0, 0) X(1, 0, 1, 0, SP_RT, 0, 0) \
  X(0, 0, 0, 1, SP_RT, 0, 0) X(0, 0, 0, 0, SP_RT, 0, 0) X(1, 1, 0, 0, SP_RT, 0, 0) X(1, 0, 0, 1, SP_RT, 0, 0) X(1, 0, 0, 0, SP_RT, 0, 0)
#define GOD_MK_MC_FORMS(X) GOD_MK_SP_FORMS(X, 1, 1)
#define GOD_MK_MH_FORMS(X) GOD_MK_SP_FORMS(X, 1, 0)          // (as GOD_FORM_HALF)
#define GOD_MK_MB_FORMS_(X, nar) X(1, 1, 0, 0, SP_RT, nar, 0) X(1, 0, 0, 1, SP_RT, nar, 0) X(1, 0, 0, 0, SP_RT, nar, 0)
#define GOD_MK_MB_FORMS(X) GOD_MK_MB_FORMS_(X, 0) GOD_MK_MB_FORMS_(X, 1)
#define GOD_VP_SP_FORMS(X, bc, cols) X(bc, 0, 0, 1, SP_MINION, 0, cols) X(bc, 0, 0, 1, 0, 0, cols)
#define GOD_VP_M_FORMS(X) GOD_VP_SP_FORMS(X, 0, 0) GOD_VP_SP_FORMS(X, 1, 0) X(0, 0, 0, 0, SP_RT, 0, 0) X(1, 1, 0, 0, SP_RT, 0, 0) X(1, 0, 0, 0, SP_RT, 0, 0)
#define GOD_VP_MC_FORMS(X) GOD_VP_SP_FORMS(X, 1, 1)
#define GOD_VP_MB_FORMS_(X, nar) X(0, 0, 0, 1, SP_RT, nar, 0) X(0, 0, 0, 0, SP_RT, nar, 0) X(1, 1, 0, 0, SP_RT, nar, 0) X(1, 0, 0, 1, SP_RT, nar, 0) X(1, 0, 0, 0, SP_RT, nar, 0)
#define GOD_VP_MB_FORMS(X) GOD_VP_MB_FORMS_(X, 0) GOD_VP_MB_FORMS_(X, 1)
// The form of a launch from what the host knows.  any: a face of the box (batched: of any box) carries a rule; inflow: one of them is an inlet; p2: the
// power-of-two spacings; cols: the column grid applies (god_grid_cols); batched: the descriptor launch, whose caller sets nar for its narrow boxes.
// mkflux -- upd: the update rides along; sp: god_mk_sp of the component; half: the box is wide enough for half workgroups (god_half_fits) -- they
// take the launches whose form admits the column grid, whether or not the box has a remainder column.
GOD_FN GodForm god_mk_form(bool any, bool inflow, bool p2, bool upd, int sp, bool cols, bool batched, bool half = false) {
  if (batched) return GodForm{ true, inflow, false, p2 && !inflow, SP_RT, false, false, false };
  const bool bc = any, inl = any && inflow, pw2 = p2 && !inl, h = half && upd && pw2 && bc;
  return GodForm{ bc, inl, upd, pw2, upd && pw2 ? sp : SP_RT, false, upd && pw2 && bc && cols && !h, h };
}
// velpred -- minion: use_minion, the one flag its marches compile in
GOD_FN GodForm god_vp_form(bool any, bool inflow, bool p2, bool minion, bool cols, bool batched) {
  const bool bc = any, inl = any && inflow, pw2 = p2 && !inl;
  return GodForm{ bc, inl, false, pw2, pw2 && !batched ? (minion ? SP_MINION : 0) : SP_RT, false, pw2 && bc && cols && !batched, false };
}
