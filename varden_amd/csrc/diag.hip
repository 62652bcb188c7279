// diag.hip -- run diagnostics on the device: vdn_diagnostics (include/varden_amd.h).  Integrals, extrema and a finite check of the state over the COMPOSITE grid -- the
// valid cells of level n that no box of level n + 1 covers --, every cell weighted by its own dx dy dz (dm = 2: dx dy).  No reference counterpart (multifab_min_c /
// max_c of hgproject.f90:89-95 is the nearest); DESIGN.md section 20 defines every quantity.
//
// Launch form.  diag_plan.h cuts every box of the hierarchy along k into slabs of about 64 K cells and numbers them in (level, global box, k) order.  One launch per
// level (kk_diag): a workgroup takes one slab of a local box -- per-thread accumulation over the slab's cells in the thread -> cell map, the shuffle tree inside each
// wave and the tree over the four waves of composite.h -- and stores ONE partial per quantity into the slab's slot of a partials array indexed by the global slab number.
// Sums are doubles; an extremum travels as the order-preserving 64-bit key of vdn_dev.h (-0 below +0; a minimum as the complement of its key, so that every extremum
// is a maximum and an empty slab is 0), cut into two 32-bit halves that a double holds exactly.  Several ranks: the slots of foreign boxes are zero and ONE sum
// all-reduce of the array fills them (x + 0 + ... + 0 is x in any order, halves and counts included).  kk_diag_final then adds the slots in slab order and takes the
// maxima of the keys, one wave per quantity (slot_sum, slot_max), and one read-back brings the 58 results home.  No floating-point atomic anywhere: the bits of a
// result depend on the box lists alone -- not on the number of ranks, not on the call; composite.h states what that rests on.
// Memory: descriptors, partials and the byte mask of covered cells live in the arena of the call's ArenaScope.  The call writes none of its inputs and,
// without VDN_DIAG_VORT, reads no ghost cell.
#include "composite.h"

namespace {
constexpr int DG_THREADS = COMP_THREADS, DG_MAXS = 11;
// sums of a slab (slots 0 .. DQ_NSUM-1 of its partial) ...
enum { DQ_CELLS = 0, DQ_NONFIN = 1, DQ_VOL = 2, DQ_S = 3, DQ_MOM = DQ_S + DG_MAXS, DQ_KIN = DQ_MOM + 3, DQ_ENS = DQ_KIN + 1, DQ_NSUM = DQ_ENS + 1 };
// ... and its extrema, two slots each (high and low half of the key)
enum { DK_SMIN = 0, DK_SMAX = DG_MAXS, DK_UMIN = 2 * DG_MAXS, DK_UMAX = DK_UMIN + 3, DK_MAGV = DK_UMAX + 3, DK_VMIN = DK_MAGV + 1, DK_VMAX = DK_VMIN + 1, DK_NKEY = DK_VMAX + 1 };
constexpr int DG_NQ = DQ_NSUM + 2 * DK_NKEY;
// what kk_diag_final leaves for the read-back: the sums, cells and volume per level, the keys
enum { DO_CELLS_LEV = DQ_NSUM, DO_VOL_LEV = DO_CELLS_LEV + VDN_MAXLEV, DO_KEYS = DO_VOL_LEV + VDN_MAXLEV, DO_N = DO_KEYS + DK_NKEY };
static_assert(DO_N <= 64, "one read_scalars brings the results home");
static_assert(DG_MAXS == 11 && VDN_MAXLEV == 4, "vdn_diag's arrays");

DEVI bool dg_finite(double v) { return fabs(v) < __builtin_huge_val(); }

template <int NS> constexpr bool dq_used(int q) { return q < DQ_S + NS || q >= DQ_MOM; }
template <int NS> constexpr bool dk_used(int q) { return q < DK_SMIN + NS || (q >= DK_SMAX && q < DK_SMAX + NS) || q >= DK_UMIN; }

// NS: the scalars the instantiation can carry (nscal <= NS; the loops over them are unrolled so that every accumulator is a register); VORT: the vorticity terms
template <int NS, bool VORT>
__global__ void __launch_bounds__(DG_THREADS) kk_diag(const CompBoxV *descs, double *__restrict__ part, int nscal, int dm, double vol) {
  const CompBoxV &D = as_constant(descs + blockIdx.x);
  const int nx = D.hi[0] - D.lo[0] + 1, ny = D.hi[1] - D.lo[1] + 1, nz = D.hi[2] - D.lo[2] + 1;
  const int tot = nx * ny * nz;
  const unsigned char *mask = D.mask;
  const FV fu = D.u, fs = D.s;
  double a[DQ_NSUM]; u64 kx[DK_NKEY];
  #pragma unroll
  for (int q = 0; q < DQ_NSUM; q++) a[q] = 0.0;
  #pragma unroll
  for (int q = 0; q < DK_NKEY; q++) kx[q] = 0;
  int ncell = 0, nbad = 0;
  // UNR cells per thread and trip: all their loads are issued before the first is used.  With one slab per compute unit (a 256^3 box: 256 slabs, one wave per
  // SIMD) the march is bound by the latency of a trip, not by bandwidth; the cells are still added in ascending order of t, so the unrolling changes no bit.
  // Covered cells and the lanes past the end load a valid cell all the same (past the end: the slab's first) and are dropped afterwards.
  constexpr int UNR = NS <= 4 ? 8 : 4;
  CellMap M(nx, ny, (int)threadIdx.x);
  for (int t0 = (int)threadIdx.x; t0 < tot; t0 += UNR * DG_THREADS) {
    double uv[UNR][3], sv[UNR][NS], wv[UNR];
    bool live[UNR];
    #pragma unroll
    for (int e = 0; e < UNR; e++) {
      live[e] = t0 + e * DG_THREADS < tot;
      const int i = D.lo[0] + (live[e] ? M.ci : 0), j = D.lo[1] + (live[e] ? M.cj : 0), k = D.lo[2] + (live[e] ? M.ck : 0);
      M.step();
      live[e] = load_cell<NS>(D, fu, fs, mask, i, j, k, live[e], nscal, dm, uv[e], sv[e]);
      wv[e] = VORT ? vort_value(fu, D.A, i, j, k) : 0.0;
    }
    #pragma unroll
    for (int e = 0; e < UNR; e++) {
      if (!live[e]) continue;
      bool fin = true;
      #pragma unroll
      for (int d = 0; d < 3; d++) fin = fin && dg_finite(uv[e][d]);
      #pragma unroll
      for (int c = 0; c < NS; c++) fin = fin && dg_finite(sv[e][c]);
      ncell++; nbad += fin ? 0 : 1;
      #pragma unroll
      for (int c = 0; c < NS; c++) if (c < nscal) {
        a[DQ_S + c] = a[DQ_S + c] + sv[e][c];
        const u64 key = key_of(sv[e][c]);
        kx[DK_SMIN + c] = key_max(kx[DK_SMIN + c], ~key); kx[DK_SMAX + c] = key_max(kx[DK_SMAX + c], key);
      }
      #pragma unroll
      for (int d = 0; d < 3; d++) if (d < dm) {
        a[DQ_MOM + d] = a[DQ_MOM + d] + sv[e][0] * uv[e][d];
        const u64 key = key_of(uv[e][d]);
        kx[DK_UMIN + d] = key_max(kx[DK_UMIN + d], ~key); kx[DK_UMAX + d] = key_max(kx[DK_UMAX + d], key);
      }
      double q2 = uv[e][0] * uv[e][0] + uv[e][1] * uv[e][1];                // magvel_value's expression (derived.h), on the values already loaded
      if (dm == 3) q2 = q2 + uv[e][2] * uv[e][2];
      a[DQ_KIN] = a[DQ_KIN] + 0.5 * sv[e][0] * q2;
      kx[DK_MAGV] = key_max(kx[DK_MAGV], key_of(sqrt(q2)));
      if (VORT) {
        a[DQ_ENS] = a[DQ_ENS] + 0.5 * wv[e] * wv[e];
        const u64 key = key_of(wv[e]);
        kx[DK_VMIN] = key_max(kx[DK_VMIN], ~key); kx[DK_VMAX] = key_max(kx[DK_VMAX], key);
      }
    }
  }
  a[DQ_CELLS] = (double)ncell; a[DQ_NONFIN] = (double)nbad; a[DQ_VOL] = (double)ncell;
  // the wave, then the four waves through LDS, one thread per quantity
  #pragma unroll
  for (int q = 0; q < DQ_NSUM; q++) if (dq_used<NS>(q)) a[q] = wave_sum(a[q]);
  #pragma unroll
  for (int q = 0; q < DK_NKEY; q++) if (dk_used<NS>(q)) kx[q] = wave_max(kx[q]);
  __shared__ WaveMeet<DQ_NSUM, DK_NKEY> sh;
  if ((threadIdx.x & 63) == 0) sh.put((int)threadIdx.x >> 6, a, kx);
  __syncthreads();
  double *out = part + (long)D.slot * DG_NQ;
  const int q = (int)threadIdx.x;
  if (q < DQ_NSUM) {
    const double v = sh.sum(q);
    out[q] = q >= DQ_VOL ? v * vol : v;
  } else if (q >= 64 && q < 64 + DK_NKEY) key_split(sh.max(q - 64), out + DQ_NSUM + 2 * (q - 64));
}

// the slots in slab order, one wave per result: wave t < DO_KEYS adds its quantity over the slots in (level, box, k) order (slot_sum), the 2 * VDN_MAXLEV waves
// after the sums add cells and volume level by level, the last DK_NKEY waves take the maxima of the keys
struct DiagLev { int start[VDN_MAXLEV + 1]; };
__global__ void __launch_bounds__(64) kk_diag_final(const double *__restrict__ part, DiagLev L, int nlev, double *__restrict__ res) {
  const int t = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (t < DO_KEYS) {
    int q = t, s0 = 0, s1 = L.start[nlev];
    if (t >= DO_CELLS_LEV) {
      const int n = (t - DO_CELLS_LEV) % VDN_MAXLEV;
      q = t >= DO_VOL_LEV ? DQ_VOL : DQ_CELLS;
      if (n < nlev) { s0 = L.start[n]; s1 = L.start[n + 1]; } else s1 = 0;
    }
    const double v = slot_sum(0.0, part, DG_NQ, q, nullptr, s0, s1, lane);
    if (lane == 0) res[t] = v;
  } else if (t < DO_N) {
    const u64 key = wave_max(slot_max(0, part, DG_NQ, DQ_NSUM + 2 * (t - DO_KEYS), nullptr, 0, L.start[nlev], lane));
    if (lane == 0) reinterpret_cast<u64 *>(res)[t] = key;
  }
}

template <int NS> void launch_diag(bool vort, int nd, const CompBoxV *d, double *part, int nscal, int dm, double vol) {
  hipStream_t st = ctx().stream;
  if (vort) hipLaunchKernelGGL((kk_diag<NS, true>), dim3(nd), dim3(DG_THREADS), 0, st, d, part, nscal, dm, vol);
  else      hipLaunchKernelGGL((kk_diag<NS, false>), dim3(nd), dim3(DG_THREADS), 0, st, d, part, nscal, dm, vol);
}
}   // namespace

extern "C" size_t vdn_diag_sizeof(void) { return sizeof(vdn_diag); }

extern "C" int vdn_diagnostics(int nlev, vdn_layout *mla, vdn_multifab *const *u, vdn_multifab *const *s, const double *dx, const vdn_bc_tower *bct, int what,
                               vdn_diag *out) {
  VDN_TRY
  const bool vort = (what & VDN_DIAG_VORT) != 0;
  composite_check("vdn_diagnostics", nlev, mla, u, s, dx, bct, vort ? "VDN_DIAG_VORT" : nullptr, false);
  REQUIRE(out, "vdn_diagnostics: null output (out)");
  const int dm = ctx().prm.dm, nscal = ctx().prm.nscal;
  hipStream_t st = ctx().stream;
  ArenaScope arena;
  DiagLev L;
  const std::vector<DiagSlab> slabs = diag_plan(nlev, mla->boxes.data(), L.start);
  const int nslab = L.start[nlev];
  REQUIRE(nslab > 0, "vdn_diagnostics: the hierarchy holds no cell");
  double *d_part = (double *)arena_alloc(sizeof(double) * DG_NQ * (size_t)nslab);
  double *d_res = (double *)arena_alloc(sizeof(double) * 64);
  const bool ranks = comm_active();
  if (ranks) HIPCHK(hipMemsetAsync(d_part, 0, sizeof(double) * DG_NQ * (size_t)nslab, st));
  for (int n = 0; n < nlev; n++) {
    const std::vector<CompPiece> mine = slab_pieces(slabs, n, mla);
    if (mine.empty()) continue;
    const CompBoxV *d_desc = composite_level_vort("vdn_diagnostics", n, nlev, mla, u, s, mine, dx, bct, vort);
    const double vol = cell_volume(dx, n, dm);
    if (nscal <= 4) launch_diag<4>(vort, (int)mine.size(), d_desc, d_part, nscal, dm, vol);
    else            launch_diag<DG_MAXS>(vort, (int)mine.size(), d_desc, d_part, nscal, dm, vol);
  }
  if (ranks) comm_allreduce_sum_dev(d_part, (size_t)DG_NQ * nslab);
  hipLaunchKernelGGL(kk_diag_final, dim3(DO_N), dim3(64), 0, st, (const double *)d_part, L, nlev, d_res);
  const double *h = read_scalars(d_res, DO_N);
  vdn_diag R; memset(&R, 0, sizeof R);
  R.cells = (long long)h[DQ_CELLS]; R.nonfinite = (long long)h[DQ_NONFIN]; R.volume = h[DQ_VOL];
  for (int n = 0; n < nlev; n++) { R.cells_lev[n] = (long long)h[DO_CELLS_LEV + n]; R.volume_lev[n] = h[DO_VOL_LEV + n]; }
  for (int c = 0; c < nscal; c++) R.sum_s[c] = h[DQ_S + c];
  for (int d = 0; d < dm; d++) R.momentum[d] = h[DQ_MOM + d];
  R.kinetic = h[DQ_KIN]; R.enstrophy = vort ? h[DQ_ENS] : 0.0;
  u64 keys[DK_NKEY]; memcpy(keys, h + DO_KEYS, sizeof keys);
  for (int c = 0; c < nscal; c++) { R.s_min[c] = extremum_value(keys[DK_SMIN + c], true); R.s_max[c] = extremum_value(keys[DK_SMAX + c], false); }
  for (int d = 0; d < dm; d++) { R.u_min[d] = extremum_value(keys[DK_UMIN + d], true); R.u_max[d] = extremum_value(keys[DK_UMAX + d], false); }
  R.magvel_max = extremum_value(keys[DK_MAGV], false);
  if (vort) { R.vort_min = extremum_value(keys[DK_VMIN], true); R.vort_max = extremum_value(keys[DK_VMAX], false); }
  arena.release();
  *out = R;
  VDN_CATCH
}
