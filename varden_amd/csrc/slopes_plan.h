// slopes_plan.h -- the tiling of the pair form of the slopes march (kk_slopes_pr in godunov.hip): which lane owns which two cells, how a range splits into
// full-width and narrow row segments, row groups and k-chunks, how many bytes of LDS a workgroup stages its planes in, and whether a box's layouts take this
// form at all.  Integers only: no HIP, no ctx(), no sw() -- the kernel and launch_slopes read it, and so does tests/cpp/slopes_plan_check.cpp with a host
// compiler, so the mapping exists in one place.
//
// A lane owns the cells (i, i + 1), i = r.lo[0] + 2 p for pair p, and moves them as one 16-byte value.  A row segment is 2^lw lanes of a wave: its first and
// last lane feed their neighbours (the pairs p - 1 and p + 1 of the segment's ends, loaded and never stored), the 2^lw - 2 lanes between them own pairs.  A
// wave carries 64 >> lw segments, one per row, a workgroup of SLP_WAVES waves SLP_WAVES * (64 >> lw) consecutive rows.  The pairs of a row go to gxm full
// segments (lw = 6, 62 pairs = 124 cells each); what is left over goes to one column of narrow segments, the narrowest power of two that holds it, so that
// the last few cells of a row do not march a wave of their own.  Tiles are numbered full ones first (x fastest), then the narrow column.
// Alignment: every 16-byte access needs an even offset of i in its array, even row and component strides and a 16-byte aligned base (slopes_pair_ok).
#pragma once
#include <cstdint>
#if defined(__HIPCC__)
#define SLP_FN __host__ __device__ inline
#else
#define SLP_FN inline
#endif

#define SLP_WAVES 8                  // waves (= full-width rows) of a workgroup
#define SLP_WG_TARGET 1024           // workgroups per component a launch should have where its planes allow (measured at 256^3: 512 slower, 1024 to 4096 alike)
#define SLP_LDS_BUDGET 40960         // bytes: four workgroups share a compute unit's 160 KB

struct SlopesPlan {
  int gxm, gy;                       // full tiles: gxm segments x gy row groups of SLP_WAVES rows
  int lwr, gyr;                      // the narrow column: segments of 2^lwr lanes, gyr row groups of SLP_WAVES * (64 >> lwr) rows (gyr = 0: no such column)
  int tiles;                         // gxm * gy + gyr, the workgroups of one k-chunk
  int klen, chunks;                  // planes per k-chunk, k-chunks
};
// what the alignment rules look at, per array: the offset of the range's first cell along x in the allocation, the row stride, the component stride (doubles) and the base address
struct SlopesLayout { long off0, n0, sc; uintptr_t base; };

SLP_FN bool slopes_layout_ok(const SlopesLayout &L) { return (L.off0 & 1) == 0 && L.off0 >= 0 && (L.n0 & 1) == 0 && (L.sc & 1) == 0 && (L.base & 15) == 0; }
// nx: cells of the range along x; lo_gap / hi_gap: cells between the range and the box-grown-by-three that loads are clamped to (2 on either side where the range
// is the box grown by one).  The feed lanes load the pairs beside the range, so both gaps are exactly 2: one whole pair, inside the allocation.
SLP_FN bool slopes_pair_ok(int nx, int lo_gap, int hi_gap, const SlopesLayout &s, const SlopesLayout &sl) {
  return nx >= 2 && (nx & 1) == 0 && lo_gap == 2 && hi_gap == 2 && s.off0 >= 2 && s.off0 + nx + 2 <= s.n0 && sl.off0 + nx <= sl.n0 && slopes_layout_ok(s) && slopes_layout_ok(sl);
}
SLP_FN int slopes_lds_bytes() { return 2 * (SLP_WAVES + 4) * 64 * 16; }      // two buffers of (rows + 2 + 2 halo rows) x 64 lanes x 16 bytes; a workgroup marches one component

// wg_target: the workgroups (per component) a launch should have at least where the planes allow (chunks of at least 8 planes: each re-loads four)
SLP_FN SlopesPlan slopes_plan(int nx, int ny, int nz, int wg_target = SLP_WG_TARGET) {
  SlopesPlan P;
  const int npairs = nx / 2;
  P.gxm = npairs / 62;
  int rem = npairs - 62 * P.gxm;
  P.lwr = 6; P.gyr = 0;
  if (rem > 30) { P.gxm++; rem = 0; }                          // more than a 32-lane segment holds: a full tile
  P.gy = P.gxm ? (ny + SLP_WAVES - 1) / SLP_WAVES : 0;
  if (rem > 0) {
    P.lwr = 2; while ((1 << P.lwr) - 2 < rem) P.lwr++;
    const int rows = SLP_WAVES * (64 >> P.lwr);
    P.gyr = (ny + rows - 1) / rows;
  }
  P.tiles = P.gxm * P.gy + P.gyr;
  int chunks = (wg_target + P.tiles - 1) / P.tiles;
  if (chunks > nz / 8) chunks = nz / 8;
  if (chunks < 1) chunks = 1;
  P.klen = (nz + chunks - 1) / chunks;
  P.chunks = (nz + P.klen - 1) / P.klen;
  return P;
}
// tile t of a k-chunk: the width of its segments (2^lw lanes), its first pair and its row group
SLP_FN void slopes_tile(const SlopesPlan &P, int t, int &lw, int &pair0, int &by) {
  const int nmain = P.gxm * P.gy;
  if (t < nmain) { lw = 6; pair0 = (t % P.gxm) * 62; by = t / P.gxm; }
  else { lw = P.lwr; pair0 = P.gxm * 62; by = t - nmain; }
}
// thread tid of a tile: its lane in the segment, its row in the workgroup; returns whether the lane owns a pair (the two outer lanes feed)
SLP_FN bool slopes_lane(int lw, int tid, int &pl, int &rr) {
  const int W = 1 << lw;
  pl = tid & (W - 1); rr = tid >> lw;
  return pl >= 1 && pl <= W - 2;
}
// the threads that also stage a halo row: the first 4 * 2^lw of the workgroup; halo h = 0, 1: the rows j0 - 2, j0 - 1; 2, 3: j0 + rows, j0 + rows + 1.
// drow: the row relative to j0, slot: the row of the staged plane it goes to (own row rr sits in slot rr + 2)
SLP_FN bool slopes_halo(int lw, int tid, int &drow, int &slot) {
  const int W = 1 << lw, rows = SLP_WAVES * (64 >> lw), h = tid >> lw;
  if (tid >= 4 * W) { drow = slot = 0; return false; }
  drow = h < 2 ? h - 2 : rows + h - 2;
  slot = h < 2 ? h : rows + h;
  return true;
}
