// tail_plan.h -- the arithmetic of the one-workgroup tail cycles that keep their levels in LDS (kk_cc_tailcycle_lds in mg_cc.hip, kk_nd_tailcycle_lds in
// mg_nd.hip): which thread owns which cell or node of a level, where each level's arrays sit in LDS, how many bytes that takes and whether a level set takes this
// form at all.  Integers only: no HIP, no ctx(), no sw() -- the kernels and the host launchers read it, and so does tests/cpp/tail_plan_check.cpp with a host
// compiler, so the mapping exists in one place.
//
// A tail level is bounded by its point count (512 cells, 729 nodes), not by its extents: 8 x 4 x 16 cells are a level, and 1 x 1 x 512 would be one with a
// 3 x 3 x 514 ghosted array.  The budget below is a fixed one; a level set above it (or outside the rules of tail_plan) keeps the body that works on global memory.
//
// Cells (TAIL_CELLS): a level of n cells per axis; its phi lives in LDS with one ghost layer, e = n + 2.  Thread t owns one cell, the cells of colour 0 first:
//   colour = t / th, q = t % th, th = ((n0 + 1) / 2) n1 n2;  k = q / (half n1), j = (q / half) % n1, i = 2 (q % half) + ((j + k + colour) & 1)
// -- pass `colour` of the red-black sweep updates exactly the cells of that colour (the order of kk_cc_bottom), and the threads of a colour are whole waves.
// One residual array without ghosts (the extents of level 0) is shared by the levels: it lives from a level's residual to the restriction that follows it.
// Nodes (TAIL_NODES): a level of n cells has n + 1 nodes per axis, thread t owns node (t % m0, (t / m0) % m1, t / (m0 m1)), m = n + 1.  Two phi arrays (the
// ping-pong of the Jacobi sweeps) and the residual per level, each with one ghost layer, e = n + 3, and the level's sigma, cells -1 .. n, n + 2 per axis.
// Periodic boxes are refused: their ghost nodes are images that a fill refreshes in front of every sweep, a phase of its own that the other body has.
#pragma once
#if defined(__HIPCC__)
#define TAIL_FN __host__ __device__ inline
#else
#define TAIL_FN inline
#endif

#define TAIL_THREADS 1024
#define TAIL_MAX_LEVELS 3            // a level above the bottom has even extents > 2, so a third level below one of 8^3 cells cannot be coarsened again
#define TAIL_LDS_DOUBLES 7680        // 60 KB of the 64 KB a workgroup may declare
#define TAIL_CELLS 0
#define TAIL_NODES 1

struct TailLevel {
  int n[3];                          // cells per axis
  int e[3];                          // extents of a ghosted array in LDS
  int phi, tmp, res, sig;            // offsets in doubles (tmp, res, sig: nodes only; cells: the shared residual array is TailPlan::res)
};
struct TailPlan {
  int kind, nlev, fits;
  TailLevel L[TAIL_MAX_LEVELS];
  int res;                           // cells: offset of the residual array, ghostless, extents of level 0
  int total;                         // doubles in use
};

TAIL_FN int tail_points(int kind, const int n[3]) { return kind == TAIL_CELLS ? n[0] * n[1] * n[2] : (n[0] + 1) * (n[1] + 1) * (n[2] + 1); }
// threads with a place in the mapping (some of them own nothing when n0 is odd: the other colour's cell of their pair lies outside)
TAIL_FN int tail_threads(int kind, const int n[3]) { return kind == TAIL_CELLS ? 2 * ((n[0] + 1) / 2) * n[1] * n[2] : tail_points(kind, n); }
// the point thread t owns; false: none.  colour: cells only
TAIL_FN bool tail_owner(int kind, const int n[3], int t, int &i, int &j, int &k, int &colour) {
  i = j = k = colour = 0;
  if (t < 0 || t >= tail_threads(kind, n)) return false;
  if (kind == TAIL_CELLS) {
    const int half = (n[0] + 1) / 2, th = half * n[1] * n[2];
    colour = t / th;
    const int q = t - colour * th;
    k = q / (half * n[1]); j = (q / half) % n[1];
    i = 2 * (q % half) + ((j + k + colour) & 1);
    if (i >= n[0]) { i = 0; return false; }
    return true;
  }
  const int m0 = n[0] + 1, m1 = n[1] + 1;
  i = t % m0; j = (t / m0) % m1; k = t / (m0 * m1);
  return true;
}
// index of cell or node (i, j, k), -1 <= i <= e - 2, in a ghosted array of the level
TAIL_FN int tail_index(const TailLevel &L, int i, int j, int k) { return (i + 1) + L.e[0] * ((j + 1) + L.e[1] * (k + 1)); }
TAIL_FN int tail_array(const TailLevel &L) { return L.e[0] * L.e[1] * L.e[2]; }

// n: the extents (cells) of the levels, finest first.  fits = 0: the level set keeps the body that works on global memory.
TAIL_FN TailPlan tail_plan(int kind, int nlev, const int (*n)[3], const int per[3]) {
  TailPlan P;
  P.kind = kind; P.nlev = nlev; P.fits = 0; P.res = 0; P.total = 0;
  for (int l = 0; l < TAIL_MAX_LEVELS; l++) for (int d = 0; d < 3; d++) { P.L[l].n[d] = P.L[l].e[d] = 0; P.L[l].phi = P.L[l].tmp = P.L[l].res = P.L[l].sig = 0; }
  if (nlev < 2 || nlev > TAIL_MAX_LEVELS) return P;
  const int g = kind == TAIL_CELLS ? 2 : 3;
  long off = 0;
  bool ok = true;
  for (int l = 0; l < nlev; l++) {
    TailLevel &L = P.L[l];
    long arr = 1;
    for (int d = 0; d < 3; d++) {
      if (n[l][d] < 1 || n[l][d] > TAIL_THREADS) return P;
      L.n[d] = n[l][d]; L.e[d] = n[l][d] + g; arr *= L.e[d];
      if (l > 0 && 2 * n[l][d] != n[l - 1][d]) ok = false;                  // every axis halves: what the restriction and the prolongation index by
      // cells: the owner of a cell next to a periodic face writes the ghost image with it, which is free of a race only when the cell across the face has
      // the other colour (an even extent).  nodes: no periodic axis
      if (per[d] && (kind == TAIL_NODES || (n[l][d] & 1))) ok = false;
    }
    if ((long)L.n[0] * L.n[1] * L.n[2] > TAIL_THREADS || tail_threads(kind, L.n) > TAIL_THREADS) return P;
    L.phi = (int)off; off += arr;
    if (kind == TAIL_NODES) { L.tmp = (int)off; off += arr; L.res = (int)off; off += arr; L.sig = (int)off; off += (long)(L.n[0] + 2) * (L.n[1] + 2) * (L.n[2] + 2); }
    if (off > TAIL_LDS_DOUBLES) return P;
  }
  if (kind == TAIL_CELLS) { P.res = (int)off; off += (long)n[0][0] * n[0][1] * n[0][2]; }
  P.total = (int)off;
  P.fits = ok && off <= TAIL_LDS_DOUBLES;
  return P;
}
TAIL_FN long tail_lds_bytes(const TailPlan &P) { return 8L * P.total; }
