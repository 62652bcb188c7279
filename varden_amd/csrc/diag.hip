// diag.hip -- run diagnostics on the device: vdn_diagnostics (include/varden_amd.h).  Integrals, extrema and a finite check of the state over the COMPOSITE grid -- the
// valid cells of level n that no box of level n + 1 covers --, every cell weighted by its own dx dy dz (dm = 2: dx dy).  No reference counterpart (multifab_min_c /
// max_c of hgproject.f90:89-95 is the nearest); DESIGN.md section 20 defines every quantity.
//
// Launch form.  diag_plan.h cuts every box of the hierarchy along k into slabs of about 64 K cells and numbers them in (level, global box, k) order.  One launch per
// level (kk_diag): a workgroup takes one slab of a local box -- per-thread accumulation over the slab's cells in a fixed thread -> cell map, a shuffle tree inside each
// wave, a fixed tree over the four waves through LDS -- and stores ONE partial per quantity into the slab's slot of a partials array indexed by the global slab number.
// Sums are doubles; an extremum travels as the order-preserving 64-bit key of fabio.hip (-0 below +0; a minimum as the complement of its key, so that every extremum
// is a maximum and an empty slab is 0), cut into two 32-bit halves that a double holds exactly.  Several ranks: the slots of foreign boxes are zero and ONE sum
// all-reduce of the array fills them (x + 0 + ... + 0 is x in any order, halves and counts included).  kk_diag_final then adds the slots in slab order and takes the
// maxima of the keys, one wave per quantity, and one read-back brings the 58 results home.  No floating-point atomic anywhere: the bits of a result depend on the box
// lists alone -- not on the number of ranks, not on the call.
// Memory: descriptors, partials and the byte mask of covered cells live in the arena between arena_mark and arena_release.  The call writes none of its inputs and,
// without VDN_DIAG_VORT, reads no ghost cell.
#include "vdn_dev.h"
#include "derived.h"
#include "diag_plan.h"

void comm_allreduce_sum_dev(double *d, size_t n);      // exchange.hip

namespace {
constexpr int DG_THREADS = 256, DG_MAXS = 11;
// sums of a slab (slots 0 .. DQ_NSUM-1 of its partial) ...
enum { DQ_CELLS = 0, DQ_NONFIN = 1, DQ_VOL = 2, DQ_S = 3, DQ_MOM = DQ_S + DG_MAXS, DQ_KIN = DQ_MOM + 3, DQ_ENS = DQ_KIN + 1, DQ_NSUM = DQ_ENS + 1 };
// ... and its extrema, two slots each (high and low half of the key)
enum { DK_SMIN = 0, DK_SMAX = DG_MAXS, DK_UMIN = 2 * DG_MAXS, DK_UMAX = DK_UMIN + 3, DK_MAGV = DK_UMAX + 3, DK_VMIN = DK_MAGV + 1, DK_VMAX = DK_VMIN + 1, DK_NKEY = DK_VMAX + 1 };
constexpr int DG_NQ = DQ_NSUM + 2 * DK_NKEY;
// what kk_diag_final leaves for the read-back: the sums, cells and volume per level, the keys
enum { DO_CELLS_LEV = DQ_NSUM, DO_VOL_LEV = DO_CELLS_LEV + VDN_MAXLEV, DO_KEYS = DO_VOL_LEV + VDN_MAXLEV, DO_N = DO_KEYS + DK_NKEY };
static_assert(DO_N <= 64, "one read_scalars brings the results home");
static_assert(DG_MAXS == 11 && VDN_MAXLEV == 4, "vdn_diag's arrays");

typedef unsigned long long u64;
DEVI u64 dg_key(double v) {                             // fabio.hip's dkey: monotone in the value, -0 below +0
  const u64 b = (u64)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
double dg_key_value(u64 k, bool is_min) {              // 0: no cell contributed
  if (k == 0) return 0.0;
  if (is_min) k = ~k;
  const u64 b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  double v; memcpy(&v, &b, 8); return v;
}
DEVI u64 dg_max(u64 a, u64 b) { return a > b ? a : b; }
DEVI bool dg_finite(double v) { return fabs(v) < __builtin_huge_val(); }

// one slab: planes lo[2] .. hi[2] of a local box; mask (or NULL): one byte per valid cell of the box, x fastest, != 0 where the next level covers the cell
struct DiagD { FV u, s; const unsigned char *mask; int lo[3], hi[3]; int blo[3], bnx, bny; int slot; VortArgs A; };

template <int NS> constexpr bool dq_used(int q) { return q < DQ_S + NS || q >= DQ_MOM; }
template <int NS> constexpr bool dk_used(int q) { return q < DK_SMIN + NS || (q >= DK_SMAX && q < DK_SMAX + NS) || q >= DK_UMIN; }

// NS: the scalars the instantiation can carry (nscal <= NS; the loops over them are unrolled so that every accumulator is a register); VORT: the vorticity terms
template <int NS, bool VORT>
__global__ void __launch_bounds__(DG_THREADS) kk_diag(const DiagD *descs, double *__restrict__ part, int nscal, int dm, double vol) {
  const DiagD &D = as_constant(descs + blockIdx.x);
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
  // The cell of index t is (t % nx, (t / nx) % ny, t / (nx ny)) from the slab's corner; a thread's cells are DG_THREADS apart, so it divides once and then steps
  // by the constants (di, dj, dk) with one carry each.
  constexpr int UNR = NS <= 4 ? 8 : 4;
  const int di = DG_THREADS % nx, dr = DG_THREADS / nx, dj = dr % ny, dk = dr / ny;
  int ci, cj, ck;                                                          // the thread's next cell, relative to the slab's corner
  { const int t = (int)threadIdx.x, r = t / nx; ci = t - r * nx; ck = r / ny; cj = r - ck * ny; }
  for (int t0 = (int)threadIdx.x; t0 < tot; t0 += UNR * DG_THREADS) {
    double uv[UNR][3], sv[UNR][NS], wv[UNR];
    bool live[UNR];
    #pragma unroll
    for (int e = 0; e < UNR; e++) {
      live[e] = t0 + e * DG_THREADS < tot;
      const int i = D.lo[0] + (live[e] ? ci : 0), j = D.lo[1] + (live[e] ? cj : 0), k = D.lo[2] + (live[e] ? ck : 0);
      { ci += di; const int c1 = ci >= nx ? 1 : 0; ci -= c1 ? nx : 0; cj += dj + c1; const int c2 = cj >= ny ? 1 : 0; cj -= c2 ? ny : 0; ck += dk + c2; }
      if (mask) live[e] = live[e] && mask[((long)(k - D.blo[2]) * D.bny + (j - D.blo[1])) * D.bnx + (i - D.blo[0])] == 0;
      const long iu = fv_idx(fu, i, j, k), is = fv_idx(fs, i, j, k);
      #pragma unroll
      for (int d = 0; d < 3; d++) uv[e][d] = d < dm ? fu.p[iu + fu.sc * d] : 0.0;
      #pragma unroll
      for (int c = 0; c < NS; c++) sv[e][c] = c < nscal ? fs.p[is + fs.sc * c] : 0.0;
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
        const u64 key = dg_key(sv[e][c]);
        kx[DK_SMIN + c] = dg_max(kx[DK_SMIN + c], ~key); kx[DK_SMAX + c] = dg_max(kx[DK_SMAX + c], key);
      }
      #pragma unroll
      for (int d = 0; d < 3; d++) if (d < dm) {
        a[DQ_MOM + d] = a[DQ_MOM + d] + sv[e][0] * uv[e][d];
        const u64 key = dg_key(uv[e][d]);
        kx[DK_UMIN + d] = dg_max(kx[DK_UMIN + d], ~key); kx[DK_UMAX + d] = dg_max(kx[DK_UMAX + d], key);
      }
      double q2 = uv[e][0] * uv[e][0] + uv[e][1] * uv[e][1];                // magvel_value's expression (derived.h), on the values already loaded
      if (dm == 3) q2 = q2 + uv[e][2] * uv[e][2];
      a[DQ_KIN] = a[DQ_KIN] + 0.5 * sv[e][0] * q2;
      kx[DK_MAGV] = dg_max(kx[DK_MAGV], dg_key(sqrt(q2)));
      if (VORT) {
        a[DQ_ENS] = a[DQ_ENS] + 0.5 * wv[e] * wv[e];
        const u64 key = dg_key(wv[e]);
        kx[DK_VMIN] = dg_max(kx[DK_VMIN], ~key); kx[DK_VMAX] = dg_max(kx[DK_VMAX], key);
      }
    }
  }
  a[DQ_CELLS] = (double)ncell; a[DQ_NONFIN] = (double)nbad; a[DQ_VOL] = (double)ncell;
  // the wave: a shuffle tree, the same for every call
  #pragma unroll
  for (int q = 0; q < DQ_NSUM; q++) if (dq_used<NS>(q)) {
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) a[q] = a[q] + __shfl_down(a[q], o, 64);
  }
  #pragma unroll
  for (int q = 0; q < DK_NKEY; q++) if (dk_used<NS>(q)) {
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) kx[q] = dg_max(kx[q], __shfl_down(kx[q], o, 64));
  }
  // the four waves: (w0 + w1) + (w2 + w3) through LDS, one thread per quantity
  __shared__ double shd[DG_THREADS / 64][DQ_NSUM];
  __shared__ u64 shk[DG_THREADS / 64][DK_NKEY];
  const int wave = (int)threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    #pragma unroll
    for (int q = 0; q < DQ_NSUM; q++) shd[wave][q] = a[q];
    #pragma unroll
    for (int q = 0; q < DK_NKEY; q++) shk[wave][q] = kx[q];
  }
  __syncthreads();
  double *out = part + (long)D.slot * DG_NQ;
  const int q = (int)threadIdx.x;
  if (q < DQ_NSUM) {
    const double v = (shd[0][q] + shd[1][q]) + (shd[2][q] + shd[3][q]);
    out[q] = q >= DQ_VOL ? v * vol : v;
  } else if (q >= 64 && q < 64 + DK_NKEY) {
    const int c = q - 64;
    const u64 key = dg_max(dg_max(shk[0][c], shk[1][c]), dg_max(shk[2][c], shk[3][c]));
    out[DQ_NSUM + 2 * c] = (double)(unsigned)(key >> 32); out[DQ_NSUM + 2 * c + 1] = (double)(unsigned)(key & 0xffffffffull);
  }
}

// the slots in slab order, one wave per result: wave t < DO_KEYS adds its quantity over the slots -- 64 slots are loaded at once, one per lane, and added lane by
// lane, so the sum runs in (level, box, k) order whatever the lanes do (a thread walking the slots alone waits for one load per slot: 0.8 ms on 2015 slabs) --, the
// 2 * VDN_MAXLEV waves after the sums add cells and volume level by level, the last DK_NKEY waves take the maxima of the keys
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
    double v = 0.0;
    for (int base = s0; base < s1; base += 64) {
      const int s = base + lane, n = s1 - base < 64 ? s1 - base : 64;
      const double x = s < s1 ? part[(long)s * DG_NQ + q] : 0.0;
      for (int l = 0; l < n; l++) v = v + __shfl(x, l, 64);
    }
    if (lane == 0) res[t] = v;
  } else if (t < DO_N) {
    const int c = t - DO_KEYS;
    u64 key = 0;
    for (int s = lane; s < L.start[nlev]; s += 64) {
      const double *p = part + (long)s * DG_NQ + DQ_NSUM + 2 * c;
      key = dg_max(key, ((u64)(unsigned)p[0] << 32) | (u64)(unsigned)p[1]);
    }
    #pragma unroll
    for (int o = 32; o > 0; o >>= 1) key = dg_max(key, __shfl_down(key, o, 64));
    if (lane == 0) reinterpret_cast<u64 *>(res)[t] = key;
  }
}

// the cells of a level that the next level covers: a byte per valid cell of every local box, set box pair by box pair (the box-batched cell launch of vdn_dev.h)
struct cover_K { unsigned char *m; int blo[3], bnx, bny;
  __device__ void cell(int i, int j, int k) const { m[((long)(k - blo[2]) * bny + (j - blo[1])) * bnx + (i - blo[0])] = 1; } };
}   // namespace
// returns the mask of every local box of level n of `mf` (arena memory); declared in vdn_internal.h: vdn_profiles (profiles.hip) masks the same cells
std::vector<unsigned char *> cover_masks(const vdn_layout *la, const vdn_multifab *mf, int n) {
  hipStream_t st = ctx().stream;
  const int nb = mf->nfabs();
  std::vector<unsigned char *> m(nb, nullptr);
  if (nb == 0) return m;
  size_t total = 0; std::vector<size_t> off(nb);
  for (int b = 0; b < nb; b++) {
    off[b] = total;
    size_t c = 1; for (int d = 0; d < 3; d++) c *= (size_t)(mf->vbox[b].hi[d] - mf->vbox[b].lo[d] + 1);
    total += (c + 63) & ~(size_t)63;
  }
  unsigned char *base = (unsigned char *)arena_alloc(total);
  HIPCHK(hipMemsetAsync(base, 0, total, st));
  for (int b = 0; b < nb; b++) m[b] = base + off[b];
  std::vector<std::pair<cover_K, Range3>> v;
  const BoxBins bins(mf->vbox);
  for (const vdn_box &f : la->boxes[n + 1]) {
    int clo[3], chi[3];
    for (int d = 0; d < 3; d++) { const int r = la->rr[3 * n + d]; clo[d] = f.lo[d] / r; chi[d] = f.hi[d] / r; }
    for (int b : bins.near(clo, chi, 0)) {
      cover_K q; Range3 r; bool any = true;
      for (int d = 0; d < 3; d++) { r.lo[d] = std::max(clo[d], mf->vbox[b].lo[d]); r.hi[d] = std::min(chi[d], mf->vbox[b].hi[d]); any = any && r.lo[d] <= r.hi[d]; q.blo[d] = mf->vbox[b].lo[d]; }
      if (!any) continue;
      q.m = m[b]; q.bnx = mf->vbox[b].hi[0] - mf->vbox[b].lo[0] + 1; q.bny = mf->vbox[b].hi[1] - mf->vbox[b].lo[1] + 1;
      v.push_back({ q, r });
    }
  }
  launch_cells(v, st);
  return m;
}
namespace {

template <int NS> void launch_diag(bool vort, int nd, const DiagD *d, double *part, int nscal, int dm, double vol) {
  hipStream_t st = ctx().stream;
  if (vort) hipLaunchKernelGGL((kk_diag<NS, true>), dim3(nd), dim3(DG_THREADS), 0, st, d, part, nscal, dm, vol);
  else      hipLaunchKernelGGL((kk_diag<NS, false>), dim3(nd), dim3(DG_THREADS), 0, st, d, part, nscal, dm, vol);
}
}   // namespace

extern "C" size_t vdn_diag_sizeof(void) { return sizeof(vdn_diag); }

extern "C" int vdn_diagnostics(int nlev, vdn_layout *mla, vdn_multifab *const *u, vdn_multifab *const *s, const double *dx, const vdn_bc_tower *bct, int what,
                               vdn_diag *out) {
  VDN_TRY
  REQUIRE(ctx().inited, "vdn_diagnostics: vdn_init has not been called");
  REQUIRE(mla && u && s && out, "vdn_diagnostics: null argument (mla, u, s, out)");
  REQUIRE(nlev >= 1 && nlev <= VDN_MAXLEV, "vdn_diagnostics: nlev = %d is outside 1 .. %d", nlev, VDN_MAXLEV);
  REQUIRE(nlev == mla->nlev, "vdn_diagnostics: nlev = %d does not match the layout's %d levels", nlev, mla->nlev);
  const int dm = ctx().prm.dm, nscal = ctx().prm.nscal;
  const bool vort = (what & VDN_DIAG_VORT) != 0;
  REQUIRE(dm == 3 || nlev == 1, "vdn_diagnostics: dm = 2 runs on one level (nlev = %d)", nlev);
  REQUIRE(dx, "vdn_diagnostics: dx is NULL (every cell is weighted by its volume%s)", vort ? "; VDN_DIAG_VORT needs it too" : "");
  REQUIRE(!vort || bct, "vdn_diagnostics: VDN_DIAG_VORT needs the bc tower (bct is NULL)");
  for (int n = 0; n < nlev; n++) {
    REQUIRE(u[n] && s[n], "vdn_diagnostics: level %d: null multifab", n);
    REQUIRE(u[n]->la == mla && s[n]->la == mla && u[n]->lev == n && s[n]->lev == n, "vdn_diagnostics: level %d: the layouts of u and s differ (from each other or from mla)", n);
    REQUIRE(u[n]->nfabs() == s[n]->nfabs(), "vdn_diagnostics: level %d: the layouts of u and s differ (%d and %d local boxes)", n, u[n]->nfabs(), s[n]->nfabs());
    REQUIRE(u[n]->nc >= dm && s[n]->nc >= nscal, "vdn_diagnostics: level %d: u carries %d components (dm = %d), s %d (nscal = %d)", n, u[n]->nc, dm, s[n]->nc, nscal);
    for (int d = 0; d < 3; d++) REQUIRE(!u[n]->nodal[d] && !s[n]->nodal[d], "vdn_diagnostics: level %d: cell-centred multifabs expected", n);
    REQUIRE(!vort || u[n]->ng >= 1, "vdn_diagnostics: level %d: VDN_DIAG_VORT reads one ghost layer of u (ng = %d)", n, u[n]->ng);
  }
  hipStream_t st = ctx().stream;
  const size_t mark = arena_mark();
  struct Giveback { size_t mark; bool armed; ~Giveback() { if (armed) ctx().arena_off = mark; } } giveback{ mark, true };     // a refusal below leaves nothing allocated either
  DiagLev L;
  const std::vector<DiagSlab> slabs = diag_plan(nlev, mla->boxes.data(), L.start);
  const int nslab = L.start[nlev];
  REQUIRE(nslab > 0, "vdn_diagnostics: the hierarchy holds no cell");
  double *d_part = (double *)arena_alloc(sizeof(double) * DG_NQ * (size_t)nslab);
  double *d_res = (double *)arena_alloc(sizeof(double) * 64);
  const bool ranks = comm_active();
  if (ranks) HIPCHK(hipMemsetAsync(d_part, 0, sizeof(double) * DG_NQ * (size_t)nslab, st));
  for (int n = 0; n < nlev; n++) {
    const std::vector<int> mine = diag_plan_local(slabs, n, mla->owner.data(), ctx().rank);
    if (mine.empty()) continue;
    std::map<int, int> local_of;                           // global box -> local index
    for (int i = 0; i < (int)mla->local[n].size(); i++) local_of[mla->local[n][i]] = i;
    std::vector<unsigned char *> mask;
    if (n < nlev - 1) mask = cover_masks(mla, u[n], n);
    std::vector<DiagD> v(mine.size());
    for (size_t q = 0; q < mine.size(); q++) {
      const DiagSlab &S = slabs[mine[q]];
      const auto it = local_of.find(S.box);
      REQUIRE(it != local_of.end() && it->second < u[n]->nfabs(), "vdn_diagnostics: level %d: box %d is not local", n, S.box);
      const int b = it->second;
      DiagD &D = v[q];
      D.u = u[n]->fabs[b]; D.s = s[n]->fabs[b]; D.mask = mask.empty() ? nullptr : mask[b]; D.slot = mine[q];
      for (int d = 0; d < 3; d++) {
        REQUIRE(u[n]->vbox[b].lo[d] == s[n]->vbox[b].lo[d] && u[n]->vbox[b].hi[d] == s[n]->vbox[b].hi[d], "vdn_diagnostics: level %d: the layouts of u and s differ", n);
        D.lo[d] = D.blo[d] = u[n]->vbox[b].lo[d]; D.hi[d] = u[n]->vbox[b].hi[d];
      }
      D.lo[2] = S.k0; D.hi[2] = S.k1;
      D.bnx = u[n]->vbox[b].hi[0] - u[n]->vbox[b].lo[0] + 1; D.bny = u[n]->vbox[b].hi[1] - u[n]->vbox[b].lo[1] + 1;
      if (vort) D.A = vort_args(u[n], b, bct, dx + 3 * n, dm, 0); else { D.A = VortArgs(); D.A.dm = dm; }
    }
    DiagD *d_desc = (DiagD *)arena_alloc(sizeof(DiagD) * v.size());
    upload_staged(d_desc, v.data(), sizeof(DiagD) * v.size());
    double vol = dx[3 * n] * dx[3 * n + 1];
    if (dm == 3) vol = vol * dx[3 * n + 2];
    if (nscal <= 4) launch_diag<4>(vort, (int)v.size(), d_desc, d_part, nscal, dm, vol);
    else            launch_diag<DG_MAXS>(vort, (int)v.size(), d_desc, d_part, nscal, dm, vol);
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
  for (int c = 0; c < nscal; c++) { R.s_min[c] = dg_key_value(keys[DK_SMIN + c], true); R.s_max[c] = dg_key_value(keys[DK_SMAX + c], false); }
  for (int d = 0; d < dm; d++) { R.u_min[d] = dg_key_value(keys[DK_UMIN + d], true); R.u_max[d] = dg_key_value(keys[DK_UMAX + d], false); }
  R.magvel_max = dg_key_value(keys[DK_MAGV], false);
  if (vort) { R.vort_min = dg_key_value(keys[DK_VMIN], true); R.vort_max = dg_key_value(keys[DK_VMAX], false); }
  giveback.armed = false;
  arena_release(mark);
  *out = R;
  VDN_CATCH
}
