// composite.h -- the pieces every reduction over the COMPOSITE grid is made of (diag.hip, profiles.hip, pdf.hip): the valid cells of level n that no box of level
// n + 1 covers.  Each piece exists here and nowhere else.
//
// The contract the three entries share: the bits of a result depend on the box lists (and the fields) alone -- not on the number of ranks, not on the call.  It
// rests on what this header fixes:
//   the map     a workgroup of COMP_THREADS threads walks the cells of its piece in the order t, t + COMP_THREADS, ...: cell t is (t % nx, (t / nx) % ny, t / (nx ny))
//               from the piece's corner (CellMap; RowMap is the same in two directions).  A thread adds its cells in ascending t whatever the unrolling.
//   the trees   wave_sum / wave_max: lane l takes lane l + 32, 16, 8, 4, 2, 1, lane 0 holds the result; the four waves meet as (w0 + w1) + (w2 + w3) (sum4, max4,
//               WaveMeet).  A maximum of keys (vdn_dev.h) is exact in any order; the tree is fixed all the same.
//   the slots   a workgroup stores ONE partial per quantity into the slot its plan names, numbered over the GLOBAL box list; foreign slots are zero and one sum
//               all-reduce fills them (x + 0 + ... + 0 is x).  slot_sum adds a run of slots in ascending order -- 64 loaded at once, one per lane, added lane by
//               lane -- and slot_max takes the maximum of their keys.
// No floating-point atomic anywhere.  The build is -ffp-contract=off -fno-fast-math, so the same operations in the same order give the same bits.
// Host side (composite.hip): the argument checks, the descriptors of a level's local pieces with the byte masks of covered cells, the cell volume.
#pragma once
#include "vdn_dev.h"
#include "derived.h"
#include "diag_plan.h"

constexpr int COMP_THREADS = 256, COMP_WAVES = COMP_THREADS / 64;

// a piece of a local box: the cells lo .. hi; mask (or NULL): one byte per valid cell of the box (corner blo, bnx x bny cells per plane), x fastest, != 0 where
// the next level covers the cell; slot: the piece's (first) place in the array of partials
struct CompBox { FV u, s; const unsigned char *mask; int lo[3], hi[3]; int blo[3], bnx, bny; int slot; };
struct CompBoxV : CompBox { VortArgs A; };              // ... with what vort_value reads

// ---- device ------------------------------------------------------------------------------------------------------------------------
// the thread -> cell map: thread t's cells are `stride` apart, so it divides once and then steps by the constants (di, dj, dk) with one carry each.  (ci, cj, ck):
// the next cell, relative to the piece's corner; beyond the piece's end they are no cell, and the caller loads the corner instead
struct CellMap {
  int nx, ny, di, dj, dk, ci, cj, ck;
  DEVI CellMap(int nx_, int ny_, int t, int stride = COMP_THREADS) : nx(nx_), ny(ny_) {
    const int dr = stride / nx; di = stride % nx; dj = dr % ny; dk = dr / ny;
    const int r = t / nx; ci = t - r * nx; ck = r / ny; cj = r - ck * ny;
  }
  DEVI void step() { ci += di; const int c1 = ci >= nx ? 1 : 0; ci -= c1 ? nx : 0; cj += dj + c1; const int c2 = cj >= ny ? 1 : 0; cj -= c2 ? ny : 0; ck += dk + c2; }
};
// ... in two directions: item t is (t % nx, t / nx)
struct RowMap {
  int nx, di, dr, ci, cr;
  DEVI RowMap(int nx_, int t, int stride = COMP_THREADS) : nx(nx_), di(stride % nx_), dr(stride / nx_), ci(t % nx_), cr(t / nx_) {}
  DEVI void step() { ci += di; const int c1 = ci >= nx ? 1 : 0; ci -= c1 ? nx : 0; cr += dr + c1; }
};

// whether cell (i, j, k) of the piece's box belongs to the composite grid
DEVI bool cell_open(const CompBox &D, const unsigned char *mask, int i, int j, int k) {
  return !mask || mask[((long)(k - D.blo[2]) * D.bny + (j - D.blo[1])) * D.bnx + (i - D.blo[0])] == 0;
}
// the values of cell (i, j, k), which is a valid cell of the box whatever `live` says (a dead lane loads a valid cell all the same and is dropped afterwards);
// returns live && not covered.  NS: the scalars the caller carries (nscal <= NS)
template <int NS>
DEVI bool load_cell(const CompBox &D, const FV &fu, const FV &fs, const unsigned char *mask, int i, int j, int k, bool live, int nscal, int dm, double (&u)[3], double (&s)[NS]) {
  live = live && cell_open(D, mask, i, j, k);
  const long iu = fv_idx(fu, i, j, k), is = fv_idx(fs, i, j, k);
  #pragma unroll
  for (int d = 0; d < 3; d++) u[d] = d < dm ? fu.p[iu + fu.sc * d] : 0.0;
  #pragma unroll
  for (int c = 0; c < NS; c++) s[c] = c < nscal ? fs.p[is + fs.sc * c] : 0.0;
  return live;
}

// the wave: a shuffle tree, the same for every call; lane 0 holds the result
DEVI double wave_sum(double x) {
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = x + __shfl_down(x, o, 64);
  return x;
}
DEVI u64 wave_max(u64 k) {
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) k = key_max(k, __shfl_down(k, o, 64));
  return k;
}
// the four waves
DEVI double sum4(double w0, double w1, double w2, double w3) { return (w0 + w1) + (w2 + w3); }
DEVI u64 max4(u64 w0, u64 w1, u64 w2, u64 w3) { return key_max(key_max(w0, w1), key_max(w2, w3)); }
// ... through LDS, for the NSUM sums and NKEY keys lane 0 of every wave holds: put, __syncthreads, then one thread per quantity
template <int NSUM, int NKEY> struct WaveMeet {
  double d[COMP_WAVES][NSUM]; u64 k[COMP_WAVES][NKEY];
  DEVI void put(int wave, const double (&a)[NSUM], const u64 (&kx)[NKEY]) {
    #pragma unroll
    for (int q = 0; q < NSUM; q++) d[wave][q] = a[q];
    #pragma unroll
    for (int q = 0; q < NKEY; q++) k[wave][q] = kx[q];
  }
  DEVI double sum(int q) const { return sum4(d[0][q], d[1][q], d[2][q], d[3][q]); }
  DEVI u64 max(int c) const { return max4(k[0][c], k[1][c], k[2][c], k[3][c]); }
};

// v + part[slot * stride + col] over the slots s0 .. s1 - 1 in ascending order, by one wave: 64 are loaded at once, one per lane, and added lane by lane, so the sum
// runs in slot order whatever the lanes do (a thread walking the slots alone waits for one load per slot: 0.8 ms on 2015 slabs).  idx (or NULL): the slots are
// idx[s0 .. s1 - 1].  Every lane returns the sum
DEVI double slot_sum(double v, const double *__restrict__ part, long stride, int col, const int *__restrict__ idx, int s0, int s1, int lane) {
  for (int base = s0; base < s1; base += 64) {
    const int s = base + lane, n = s1 - base < 64 ? s1 - base : 64;
    const double x = s < s1 ? part[(long)(idx ? idx[s] : s) * stride + col] : 0.0;
    for (int l = 0; l < n; l++) v = v + __shfl(x, l, 64);
  }
  return v;
}
// the maximum of key and the keys split over part[slot * stride + col], + 1 of the same slots, lane-strided: wave_max of the lanes' results is the run's maximum
DEVI u64 slot_max(u64 key, const double *__restrict__ part, long stride, int col, const int *__restrict__ idx, int s0, int s1, int lane) {
  for (int s = s0 + lane; s < s1; s += 64) key = key_max(key, key_join(part + (long)(idx ? idx[s] : s) * stride + col));
  return key;
}

// ---- host (composite.hip) ----------------------------------------------------------------------------------------------------------
// the extremum behind a key that went through max4 / slot_max (a minimum travels as the complement of its key, so that every extremum is a maximum); 0: no cell
// contributed
__host__ __device__ inline double extremum_value(u64 k, bool is_min) { return k == 0 ? 0.0 : key_value(is_min ? ~k : k); }

// what every entry asks of (nlev, mla, u, s, dx, bct); `name` starts every message.  vort (or NULL): the name of the option that makes the call compute the
// vorticity, which needs bct and one ghost layer of u; ratio2: refuse a refinement ratio other than 2
void composite_check(const char *name, int nlev, const vdn_layout *mla, vdn_multifab *const *u, vdn_multifab *const *s, const double *dx, const vdn_bc_tower *bct,
                     const char *vort, bool ratio2);
// a plan's entry that this rank owns: the cells lo .. hi of GLOBAL box `box` of the level, its slot
struct CompPiece { int box, lo[3], hi[3], slot; };
// the descriptors of level n's pieces on the device (arena memory), in the order given: finds every piece's local box, checks that u and s agree on it and that
// the piece lies inside, builds the masks of covered cells when n < nlev - 1.  _vort: vort_args of the box when `vort`, else A.dm alone
const CompBox  *composite_level(const char *name, int n, int nlev, const vdn_layout *mla, vdn_multifab *const *u, vdn_multifab *const *s, const std::vector<CompPiece> &pieces);
const CompBoxV *composite_level_vort(const char *name, int n, int nlev, const vdn_layout *mla, vdn_multifab *const *u, vdn_multifab *const *s, const std::vector<CompPiece> &pieces,
                                     const double *dx, const vdn_bc_tower *bct, bool vort);
// the slabs of diag_plan.h that this rank owns on level n, as pieces: slab q is planes k0 .. k1 of its box, its slot is its global number
std::vector<CompPiece> slab_pieces(const std::vector<DiagSlab> &slabs, int n, const vdn_layout *mla);
double cell_volume(const double *dx, int n, int dm);
