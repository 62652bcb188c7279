// dim2.hip -- the dm = 2 path of advance_timestep (BASELINE.json configs[0], the reference's CPU-runnable case).
//
// Reference routines restated (ONE level made of any list of boxes, on one or several ranks -- the 2-D configuration is plumbing, not a
// performance target):
//   mkvelforce_2d / mkscalforce_2d   src/mkforce.f90:82-142, 290-331
//   update_2d                        src/update.f90:113-184
//   estdt_2d                         src/estdt.f90:89-129
//   divumac_2d, mk_mac_coeffs_2d, mkumac_2d      src/macproject.f90:226-248, 338-359, 538-576
//   create_uvec_2d, mkgphi_2d, hg_update_2d      src/hgproject.f90:374-432, 517-541, 581-636
//   explicit diffusive term / visc_solve / diff_scalar_solve with the 2-D right-hand sides (viscsolve.f90:226-262)
// velpred_2d / mkflux_2d live in godunov.hip.  The two elliptic solvers are compact 2-D versions of the algorithms of
// mg_cc.hip / mg_nd.hip (5-point red-black Gauss-Seidel V-cycles; 9-point Q1 damped-Jacobi V-cycles), in the expression
// order of the oracle's dm = 2 mode (oracle/vo_macproject.c, oracle/vo_hgproject.c).
//
// Box lists: the pointwise stages run on every local box, one batched launch per stage (vdn_dev.h: launch_cells).  The two solvers
// run on a GATHERED level: a private whole-domain array that the load launches fill from every local box and the store launches write
// back to every local box (valid region and ghost layer), so the V-cycles themselves do not know about boxes -- and their arithmetic and
// its order do not depend on the decomposition: phi is the same bit for bit on one box or many.  Every point of the domain array has ONE
// writer box (a face or node that two boxes share comes from the box on its high side; the domain's high faces / nodes and the ghost ring
// from the box that touches them), so nothing depends on two copies of a shared face being equal.  Several ranks: each rank loads its own
// boxes into a zeroed array and a byte-wise MAX all-reduce completes it (the owner's bytes against zeros: the owner's value, exactly);
// every rank then holds the same array and runs the same V-cycles, norms included -- no further reduction.  Memory: one whole level per
// rank (a 4096^2 level: about 1 GB for the cell-centred solver's arrays and levels), which bounds the 2-D problems this path takes.
//
// Device layout of a 2-D fab: the 3-D layout with ONE valid z-plane (k = 0); its z-ghost planes exist but are never
// read or written here (nor moved by the ghost exchange, exchange.hip: xboxes_of).  vdn_multifab_copy_to/from_host present the
// BoxLib 2-D layout p(lo1-ng:hi1+ng, lo2-ng:hi2+ng, nc).
#include "vdn_dev.h"
#include "mg_stop.h"
#include "krylov_grid.h"
#include <vector>
#include <algorithm>

#define G2(f, i, j, c) fv_get(f, i, j, 0, c)
#define P2(f, i, j, c) fv_at(f, i, j, 0, c)
static const dim3 B2(64, 4, 1);
static Range3 rng2(int lo0, int hi0, int lo1, int hi1) { Range3 r; r.lo[0] = lo0; r.hi[0] = hi0; r.lo[1] = lo1; r.hi[1] = hi1; r.lo[2] = r.hi[2] = 0; return r; }
// the 2-D solvers take one level whose boxes cover the domain (advance_timestep refuses dm = 2 hierarchies)
static void require_2d(const vdn_multifab *mf, const char *who) {
  const vdn_layout *la = mf->la;
  REQUIRE(la->nlev == 1 && mf->lev == 0, "%s: the dm = 2 path supports one level (of any list of boxes)", who);
  long cells = 0;
  for (const vdn_box &b : la->boxes[0]) cells += (long)(b.hi[0] - b.lo[0] + 1) * (b.hi[1] - b.lo[1] + 1);
  const vdn_box &pd = la->pd[0];
  REQUIRE(cells == (long)(pd.hi[0] - pd.lo[0] + 1) * (pd.hi[1] - pd.lo[1] + 1), "%s: the boxes of a dm = 2 level must cover its domain", who);
}
template <class K> static void run_cells(const std::vector<std::pair<K, Range3>> &v) { launch_cells(v, ctx().stream); }

// ---- forcing, update, estdt -------------------------------------------------------------------------------------------
struct F2Args { int lo[2], hi[2]; double coef, fac; int boussinesq, nscal; };
struct mkvelforce2_K { FV vf, ext, gp, s, lapu; int has_lapu; F2Args A;
  __device__ void cell(int i, int j, int) const {
    const int out = (i < A.lo[0]) + (i > A.hi[0]) + (j < A.lo[1]) + (j > A.hi[1]);
    if (out > 1) return;                               // the four edge halos only (mkforce.f90:118-139)
    const int ic = min(max(i, A.lo[0]), A.hi[0]), jc = min(max(j, A.lo[1]), A.hi[1]);
    const double rho = G2(s, i, j, 0);
    #pragma unroll
    for (int m = 0; m < 2; m++) {
      const double l = has_lapu ? G2(lapu, ic, jc, m) : 0.0;
      const double lapu_local = A.coef * A.fac * l;
      double e = G2(ext, i, j, m);
      if (out == 0 && A.boussinesq == 1) e = G2(s, i, j, 1) * e;
      P2(vf, i, j, m) = e + (lapu_local - G2(gp, i, j, m)) / rho;
    }
  } };
struct mkscalforce2_K { FV sf, ext, laps; int has_laps; F2Args A;
  __device__ void cell(int i, int j, int) const {
    const int out = (i < A.lo[0]) + (i > A.hi[0]) + (j < A.lo[1]) + (j > A.hi[1]);
    if (out > 1) return;
    const int ic = min(max(i, A.lo[0]), A.hi[0]), jc = min(max(j, A.lo[1]), A.hi[1]);
    for (int m = 1; m < A.nscal; m++) {
      const double l = has_laps ? G2(laps, ic, jc, m) : 0.0;
      P2(sf, i, j, m) = G2(ext, i, j, m) + A.coef * A.fac * l;
    }
  } };
void k2_mkvelforce(vdn_multifab *vf, const vdn_multifab *ext, const vdn_multifab *s, const vdn_multifab *gp, const vdn_multifab *lapu, double visc_fac) {
  mf_setval(vf, 0.0, 0, vf->nc, true);
  std::vector<std::pair<mkvelforce2_K, Range3>> v;
  for (int b = 0; b < vf->nfabs(); b++) {
    F2Args A; const vdn_box &bx = vf->vbox[b];
    for (int d = 0; d < 2; d++) { A.lo[d] = bx.lo[d]; A.hi[d] = bx.hi[d]; }
    A.coef = ctx().prm.visc_coef; A.fac = visc_fac; A.boussinesq = ctx().prm.boussinesq; A.nscal = ctx().prm.nscal;
    mkvelforce2_K K{ vf->fabs[b], ext->fabs[b], gp->fabs[b], s->fabs[b], lapu ? lapu->fabs[b] : vf->fabs[b], lapu ? 1 : 0, A };
    v.push_back({ K, rng2(A.lo[0] - 1, A.hi[0] + 1, A.lo[1] - 1, A.hi[1] + 1) });
  }
  run_cells(v);
}
void k2_mkscalforce(vdn_multifab *sf, const vdn_multifab *ext, const vdn_multifab *laps, double diff_fac) {
  mf_setval(sf, 0.0, 0, sf->nc, true);
  std::vector<std::pair<mkscalforce2_K, Range3>> v;
  for (int b = 0; b < sf->nfabs(); b++) {
    F2Args A; const vdn_box &bx = sf->vbox[b];
    for (int d = 0; d < 2; d++) { A.lo[d] = bx.lo[d]; A.hi[d] = bx.hi[d]; }
    A.coef = ctx().prm.diff_coef; A.fac = diff_fac; A.boussinesq = 0; A.nscal = ctx().prm.nscal;
    mkscalforce2_K K{ sf->fabs[b], ext->fabs[b], laps ? laps->fabs[b] : sf->fabs[b], laps ? 1 : 0, A };
    v.push_back({ K, rng2(A.lo[0] - 1, A.hi[0] + 1, A.lo[1] - 1, A.hi[1] + 1) });
  }
  run_cells(v);
}

struct U2Args { double dx[2], dt; int ncomp; int cons[VDN_MAXCOMP]; };
struct update2_K { FV sold, snew, um, vm, sx, sy, fx, fy, force; U2Args A;
  __device__ void cell(int i, int j, int) const {
    const double ubar = 0.5 * (G2(um, i, j, 0) + G2(um, i + 1, j, 0));
    const double vbar = 0.5 * (G2(vm, i, j, 0) + G2(vm, i, j + 1, 0));
    for (int c = 0; c < A.ncomp; c++) {
      const double so = G2(sold, i, j, c), f = G2(force, i, j, c);
      double v;
      if (A.cons[c]) {
        const double divsu = (G2(fx, i + 1, j, c) - G2(fx, i, j, c)) / A.dx[0] + (G2(fy, i, j + 1, c) - G2(fy, i, j, c)) / A.dx[1];
        v = so - A.dt * divsu + A.dt * f;
      } else {
        const double ug = ubar * (G2(sx, i + 1, j, c) - G2(sx, i, j, c)) / A.dx[0] + vbar * (G2(sy, i, j + 1, c) - G2(sy, i, j, c)) / A.dx[1];
        v = so - A.dt * ug + A.dt * f;
      }
      P2(snew, i, j, c) = v;
    }
  } };
void k2_update(const vdn_multifab *sold, vdn_multifab **umac, vdn_multifab **sedge, vdn_multifab **flux, const vdn_multifab *force, vdn_multifab *snew,
               const double *dx, double dt, bool is_vel, const int *is_cons) {
  U2Args A; A.dx[0] = dx[0]; A.dx[1] = dx[1]; A.dt = dt; A.ncomp = sold->nc;
  for (int c = 0; c < sold->nc; c++) A.cons[c] = (!is_vel && is_cons[c]) ? 1 : 0;
  std::vector<std::pair<update2_K, Range3>> v;
  for (int b = 0; b < sold->nfabs(); b++) {
    const vdn_box &bx = sold->vbox[b];
    update2_K K{ sold->fabs[b], snew->fabs[b], umac[0]->fabs[b], umac[1]->fabs[b], sedge[0]->fabs[b], sedge[1]->fabs[b], flux[0]->fabs[b], flux[1]->fabs[b], force->fabs[b], A };
    v.push_back({ K, rng2(bx.lo[0], bx.hi[0], bx.lo[1], bx.hi[1]) });
  }
  run_cells(v);
}
DEVI void estdt2_cell(const FV &u, const FV &s, const FV &gp, const FV &ext, int i, int j, double m[4]) {
  const double rho = G2(s, i, j, 0);
  #pragma unroll
  for (int c = 0; c < 2; c++) { m[c] = fabs(G2(u, i, j, c)); m[2 + c] = fabs(G2(gp, i, j, c) / rho - G2(ext, i, j, c)); }
}
__global__ void kk2_estdt(FV u, FV s, FV gp, FV ext, Range3 r, double *out6) {
  REDUCE_IJ(r)
  double m[4] = { 0, 0, 0, 0 };
  if (in_ij) estdt2_cell(u, s, gp, ext, i, j, m);
  block_atomic_max(out6 + 0, m[0]); block_atomic_max(out6 + 1, m[1]); block_atomic_max(out6 + 3, m[2]); block_atomic_max(out6 + 4, m[3]);
}
// several boxes: one launch, 64 x 4 tiles per box (the per-box kernel's), a workgroup finds its box by bisection
struct Est2B { Range3 r; int g[2]; FV u, s, gp, ext; };
__global__ void __launch_bounds__(256) kk2_estdt_b(const Est2B *args, const int *start, int nbox, double *out6) {
  int lo = 0, hi = nbox - 1;
  const int bid = (int)blockIdx.x;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (as_constant(start + mid) <= bid) lo = mid; else hi = mid - 1; }
  const Est2B &a = as_constant(args + lo);
  const int lb = bid - as_constant(start + lo);
  const int i = a.r.lo[0] + (lb % a.g[0]) * 64 + (int)threadIdx.x, j = a.r.lo[1] + (lb / a.g[0]) * 4 + (int)threadIdx.y;
  double m[4] = { 0, 0, 0, 0 };
  if (i <= a.r.hi[0] && j <= a.r.hi[1]) estdt2_cell(a.u, a.s, a.gp, a.ext, i, j, m);
  block_atomic_max(out6 + 0, m[0]); block_atomic_max(out6 + 1, m[1]); block_atomic_max(out6 + 3, m[2]); block_atomic_max(out6 + 4, m[3]);
}
void k2_estdt_max(const vdn_multifab *u, const vdn_multifab *s, const vdn_multifab *gp, const vdn_multifab *ext, double out6[6]) {
  VdnCtx &c = ctx();
  HIPCHK(hipMemsetAsync(c.d_scal, 0, 6 * sizeof(double), c.stream));
  const int nb = u->nfabs();
  if (nb == 1) {
    const vdn_box &bx = u->vbox[0];
    Range3 r = rng2(bx.lo[0], bx.hi[0], bx.lo[1], bx.hi[1]);
    hipLaunchKernelGGL(kk2_estdt, reduce_grid(r), B2, 0, c.stream, u->fabs[0], s->fabs[0], gp->fabs[0], ext->fabs[0], r, c.d_scal);
  } else if (nb > 1) {
    std::vector<Est2B> v(nb); std::vector<int> start(nb); int tot = 0;
    for (int b = 0; b < nb; b++) {
      Est2B &a = v[b]; const vdn_box &bx = u->vbox[b];
      a.r = rng2(bx.lo[0], bx.hi[0], bx.lo[1], bx.hi[1]);
      a.g[0] = (bx.hi[0] - bx.lo[0] + 64) / 64; a.g[1] = (bx.hi[1] - bx.lo[1] + 4) / 4;
      a.u = u->fabs[b]; a.s = s->fabs[b]; a.gp = gp->fabs[b]; a.ext = ext->fabs[b];
      start[b] = tot; tot += a.g[0] * a.g[1];
    }
    Est2B *d_args = (Est2B *)desc_scratch(sizeof(Est2B) * nb); int *d_start = (int *)desc_scratch(sizeof(int) * nb);
    upload_staged(d_args, v.data(), sizeof(Est2B) * nb); upload_staged(d_start, start.data(), sizeof(int) * nb);
    hipLaunchKernelGGL(kk2_estdt_b, dim3(tot), B2, 0, c.stream, (const Est2B *)d_args, (const int *)d_start, nb, c.d_scal);
  }
  comm_allreduce_max_dev(c.d_scal, 6);        // every rank the same dt (MAX of the maxima == the reference's MIN over ranks of dt_proc)
  HIPCHK(hipMemcpyAsync(c.h_scal, c.d_scal, 6 * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  HIPCHK(hipStreamSynchronize(c.stream));
  for (int k = 0; k < 6; k++) out6[k] = c.h_scal[k];
}

// =====================================================================================================================
// cell-centred multigrid, 5-point (alpha - div b grad) phi = rh
// =====================================================================================================================
struct C2 { int n0, n1, P; double hi2[2]; double *phi, *rh, *res, *bx, *by, *alpha; };
DEVI long c2i(const C2 &L, int i, int j) { return (long)(i + 1) + (long)L.P * (j + 1); }
KRY_HD long c2_size(int n0, int n1) { return (long)(n0 + 2) * (n1 + 2); }
DEVI void c2_apply(const C2 &L, int i, int j, double &Ap, double &diag) {
  const long c = c2i(L, i, j);
  const double p0 = L.phi[c];
  const double bxm = L.bx[c], bxp = L.bx[c + 1], bym = L.by[c], byp = L.by[c + L.P];
  const double ax = (bxp * (p0 - L.phi[c + 1]) + bxm * (p0 - L.phi[c - 1])) * L.hi2[0];
  const double ay = (byp * (p0 - L.phi[c + L.P]) + bym * (p0 - L.phi[c - L.P])) * L.hi2[1];
  Ap = ax + ay;
  diag = (bxp + bxm) * L.hi2[0] + (byp + bym) * L.hi2[1];
  if (L.alpha) { const double a0 = L.alpha[c]; Ap = Ap + a0 * p0; diag = diag + a0; }
}
__global__ void kk_c2_gsrb(C2 L, int color) {
  const int j = blockIdx.y * blockDim.y + threadIdx.y;
  const int i = 2 * (int)(blockIdx.x * blockDim.x + threadIdx.x) + ((j + color) & 1);
  if (i >= L.n0 || j >= L.n1) return;
  double Ap, diag; c2_apply(L, i, j, Ap, diag);
  const long c = c2i(L, i, j);
  if (diag != 0.0) L.phi[c] = L.phi[c] + (L.rh[c] - Ap) / diag;
}
__global__ void kk_c2_residual(C2 L, double *nrm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  double r = 0.0;
  if (i < L.n0 && j < L.n1) { double Ap, diag; c2_apply(L, i, j, Ap, diag); r = L.rh[c2i(L, i, j)] - Ap; L.res[c2i(L, i, j)] = r; }
  if (nrm) block_atomic_max(nrm, fabs(r));
}
__global__ void kk_c2_restrict(C2 F, C2 C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= C.n0 || j >= C.n1) return;
  const long f = c2i(F, 2 * i, 2 * j);
  C.rh[c2i(C, i, j)] = (F.res[f] + F.res[f + 1] + F.res[f + F.P] + F.res[f + F.P + 1]) * 0.25;
}
__global__ void kk_c2_prolong(C2 F, C2 C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= F.n0 || j >= F.n1) return;
  F.phi[c2i(F, i, j)] = F.phi[c2i(F, i, j)] + C.phi[c2i(C, i / 2, j / 2)];
}
__global__ void kk_c2_coarsen(C2 F, C2 C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i > C.n0 || j > C.n1) return;
  if (j < C.n1) C.bx[c2i(C, i, j)] = (F.bx[c2i(F, 2 * i, 2 * j)] + F.bx[c2i(F, 2 * i, 2 * j + 1)]) * 0.5;
  if (i < C.n0) C.by[c2i(C, i, j)] = (F.by[c2i(F, 2 * i, 2 * j)] + F.by[c2i(F, 2 * i + 1, 2 * j)]) * 0.5;
  if (C.alpha && i < C.n0 && j < C.n1) {
    const long f = c2i(F, 2 * i, 2 * j);
    C.alpha[c2i(C, i, j)] = (F.alpha[f] + F.alpha[f + 1] + F.alpha[f + F.P] + F.alpha[f + F.P + 1]) * 0.25;
  }
}
// entry (i, j) of the level grown by one: a ghost entry along a periodic direction takes its image (the source is a cell of the level, never a ghost: no thread
// reads what another writes)
DEVI void c2_periodic_entry(const C2 &L, int per0, int per1, int i, int j) {
  int si = i, sj = j; bool g = false, ok = true;
  if (i < 0) { g = true; if (per0) si = i + L.n0; else ok = false; } else if (i >= L.n0) { g = true; if (per0) si = i - L.n0; else ok = false; }
  if (j < 0) { g = true; if (per1) sj = j + L.n1; else ok = false; } else if (j >= L.n1) { g = true; if (per1) sj = j - L.n1; else ok = false; }
  if (g && ok) L.phi[c2i(L, i, j)] = L.phi[c2i(L, si, sj)];
}
__global__ void kk_c2_periodic(C2 L, int per0, int per1) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x) - 1, j = (int)(blockIdx.y * blockDim.y + threadIdx.y) - 1;
  if (i > L.n0 || j > L.n1) return;
  c2_periodic_entry(L, per0, per1, i, j);
}
// ---- Krylov bottom solver (vdn_params.mg_bottom_solver = 1, 2, 3; krylov_wg.h) -- the 2-D counterpart of mg_cc.hip's CcKrylov ----
// The V-cycles stop where an extent turns odd (200 -> 100 -> 50 -> 25) and there is no one-workgroup sweep kernel in this file: the 25^2 bottom takes
// max(mg_nub, N^2) = 625 red-black sweeps of two to four launches each.  CG or BiCGStab by ONE workgroup in ONE launch takes their place.  c2_apply and the
// level's arrays are used as they are; the Neumann / Dirichlet closures sit in bx / by and rely on ghost entries that read as zero (wg_krylov zeroes its
// work arrays of the padded size c2_size; the periodic fill writes ghosts only along a periodic direction).  A bottom of VDN_KRYLOV_GRID_MIN_POINTS_2D cells
// or more (n_cell = 1000: 125^2) is too much for one workgroup: there the same iteration runs over the whole GPU (krylov_grid.h).
DEVI void wg_c2_periodic(const C2 &L, int per0, int per1) {      // kk_c2_periodic by one workgroup; nothing without a periodic direction, else ends in a barrier
  if (!per0 && !per1) return;
  const int nx = L.n0 + 2, np = nx * (L.n1 + 2);
  for (int t = threadIdx.x; t < np; t += blockDim.x) c2_periodic_entry(L, per0, per1, t % nx - 1, t / nx - 1);
  __syncthreads();
}
// ... one ghost entry at a time, for the grid-wide form (krylov_grid.h): the 2 n1 entries beside the x faces when x is periodic, then the 2 n0 beside the y faces
// when y is.  The corners wg_c2_periodic also writes are left out: the 5-point operator never reads them.  The source is a cell of the level, never a ghost.
KRY_HD int c2_periodic_count(int n0, int n1, int per0, int per1) { return (per0 ? 2 * n1 : 0) + (per1 ? 2 * n0 : 0); }
DEVI void c2_periodic_point(const C2 &L, int per0, int t) {
  const int nx = per0 ? 2 * L.n1 : 0;
  int i, j, si, sj;
  if (t < nx) { j = sj = t >> 1; i = (t & 1) ? L.n0 : -1; si = (t & 1) ? 0 : L.n0 - 1; }
  else { const int u = t - nx; i = si = u >> 1; j = (u & 1) ? L.n1 : -1; sj = (u & 1) ? 0 : L.n1 - 1; }
  L.phi[c2i(L, i, j)] = L.phi[c2i(L, si, sj)];
}
// the level as wg_krylov, the grid-wide kernels and the host (mg_krylov_visit) take it (krylov_wg.h): by value
struct C2Krylov {
  C2 L; int per0, per1, sing;
  KRY_HD int count() const { return L.n0 * L.n1; }
  DEVI bool point(int t, long &c, int &i, int &j, int &k) const { i = t % L.n0; j = t / L.n0; k = 0; c = c2i(L, i, j); return true; }
  DEVI void apply(const double *v, long, int i, int j, int, double &Av, double &diag) const { C2 Lv = L; Lv.phi = const_cast<double *>(v); c2_apply(Lv, i, j, Av, diag); }
  DEVI void fill(double *v) const { C2 Lv = L; Lv.phi = v; wg_c2_periodic(Lv, per0, per1); }
  KRY_HD int fill_count() const { return c2_periodic_count(L.n0, L.n1, per0, per1); }
  DEVI void fill_point(double *v, int t) const { C2 Lv = L; Lv.phi = v; c2_periodic_point(Lv, per0, t); }
  KRY_HD long size() const { return c2_size(L.n0, L.n1); }
  DEVI const double *rhs() const { return L.rh; }
  DEVI double *x() const { return L.phi; }
  KRY_HD bool singular() const { return sing != 0; }
};
struct C2Bc { int e[2][2]; int lo[2]; };               // elliptic boundary codes of the DOMAIN faces; lo: the domain's first cell
struct C2Gx { C2 L; C2Bc B; int has_alpha; };           // what every box's load / store launch shares (kk_batched's `extra`)
// The per-box descriptors of the gathered level (vdn_dev.h: kk_batched).  r: the points THIS box writes -- each point of the domain
// array has one writer (require_2d: the boxes tile the domain).  hi: the box's last cell.
// level 0: face coefficients with the boundary folding (Neumann b := 0, Dirichlet b := 2b), alpha.  r = the box's cells, grown by one
// face at the domain's high sides: a face that two boxes share comes from the box on its high side.
struct C2LoadB { Range3 r; int g[3]; FV bxf, byf, af; int hi[2];
  static __device__ double body(const C2LoadB &q, int gi, int gj, int, const C2Gx &x) {
    const C2 &L = x.L; const C2Bc &B = x.B;
    const int i = gi - B.lo[0], j = gj - B.lo[1];
    if (gj <= q.hi[1]) {
      double v = G2(q.bxf, gi, gj, 0);
      const int side = (i == 0) ? 0 : ((i == L.n0) ? 1 : -1);
      if (side >= 0) { if (B.e[0][side] == VDN_BC_NEU) v = 0.0; else if (B.e[0][side] == VDN_BC_DIR) v = 2.0 * v; }
      L.bx[c2i(L, i, j)] = v;
    }
    if (gi <= q.hi[0]) {
      double v = G2(q.byf, gi, gj, 0);
      const int side = (j == 0) ? 0 : ((j == L.n1) ? 1 : -1);
      if (side >= 0) { if (B.e[1][side] == VDN_BC_NEU) v = 0.0; else if (B.e[1][side] == VDN_BC_DIR) v = 2.0 * v; }
      L.by[c2i(L, i, j)] = v;
    }
    if (x.has_alpha && gi <= q.hi[0] && gj <= q.hi[1]) L.alpha[c2i(L, i, j)] = G2(q.af, gi, gj, 0);
    return 0.0;
  } };
// right-hand side with the Dirichlet data (ghost cells of the incoming phi = boundary-face values) moved into it; phi.  r = the box's
// cells; returns |rh| for the norm
struct C2LoadRh { Range3 r; int g[3]; FV rh, phi;
  static __device__ double body(const C2LoadRh &q, int gi, int gj, int, const C2Gx &x) {
    const C2 &L = x.L; const C2Bc &B = x.B;
    const int i = gi - B.lo[0], j = gj - B.lo[1];
    double r = G2(q.rh, gi, gj, 0);
    const double r0 = r;
    const long c = c2i(L, i, j);
    if (i == 0 && B.e[0][0] == VDN_BC_DIR)        r = r + L.bx[c] * G2(q.phi, gi - 1, gj, 0) * L.hi2[0];
    if (i == L.n0 - 1 && B.e[0][1] == VDN_BC_DIR) r = r + L.bx[c + 1] * G2(q.phi, gi + 1, gj, 0) * L.hi2[0];
    if (j == 0 && B.e[1][0] == VDN_BC_DIR)        r = r + L.by[c] * G2(q.phi, gi, gj - 1, 0) * L.hi2[1];
    if (j == L.n1 - 1 && B.e[1][1] == VDN_BC_DIR) r = r + L.by[c + L.P] * G2(q.phi, gi, gj + 1, 0) * L.hi2[1];
    L.rh[c] = r;
    L.phi[c] = G2(q.phi, gi, gj, 0);
    return fabs(r0);
  } };
// phi back into the box's fab incl. its ghost layer: inside the domain the neighbours' phi, beyond a domain face the ghost cell the
// closure implies (Neumann: phi_i, Dirichlet: -phi_i, periodic: image).  r = the box's cells grown by one
struct C2Store { Range3 r; int g[3]; FV phi;
  static __device__ double body(const C2Store &q, int gi_, int gj_, int, const C2Gx &x) {
    const C2 &L = x.L; const C2Bc &B = x.B;
    const int i = gi_ - B.lo[0], j = gj_ - B.lo[1];
    const bool gi = (i < 0 || i >= L.n0), gj = (j < 0 || j >= L.n1);
    if (gi && gj) return 0.0;                      // the domain's corners are not needed
    double v;
    if (!gi && !gj) v = L.phi[c2i(L, i, j)];
    else {
      const int d = gi ? 0 : 1, s = gi ? (i < 0 ? 0 : 1) : (j < 0 ? 0 : 1);
      const int qi = gi ? (s ? L.n0 - 1 : 0) : i, qj = gj ? (s ? L.n1 - 1 : 0) : j;
      if (B.e[d][s] == VDN_BC_NEU) v = L.phi[c2i(L, qi, qj)];
      else if (B.e[d][s] == VDN_BC_DIR) v = -L.phi[c2i(L, qi, qj)];
      else v = L.phi[c2i(L, i, j)];
    }
    P2(q.phi, gi_, gj_, 0) = v;
    return 0.0;
  } };
// several ranks: every rank has loaded its own boxes into a zeroed array; the byte-wise MAX over the ranks is then the owner's value
// (its bytes against zeros) -- the whole array on every rank, bit for bit
static void gather_level(double *base, long ndoubles) {
  if (ctx().nranks > 1) comm_allreduce_max_u8_dev((unsigned char *)base, (size_t)ndoubles * sizeof(double));
}
static dim3 g2(int nx, int ny) { return dim3((nx + 63) / 64, (ny + 3) / 4, 1); }
struct CC2MG { std::vector<C2> lev; int per[2]; double *d_nrm;
  MgKrylov kry; int kry_singular = 0; };      // Krylov bottom solver (kry.w == nullptr: the bottom sweeps; kry.part: the grid-wide form)
static void c2_gsrb(const CC2MG &M, const C2 &L, int ns) {
  hipStream_t st = ctx().stream;
  for (int s = 0; s < ns; s++) for (int col = 0; col < 2; col++) {
    if (M.per[0] || M.per[1]) hipLaunchKernelGGL(kk_c2_periodic, g2(L.n0 + 2, L.n1 + 2), B2, 0, st, L, M.per[0], M.per[1]);
    hipLaunchKernelGGL(kk_c2_gsrb, g2((L.n0 + 1) / 2, L.n1), B2, 0, st, L, col);
  }
}
static void c2_residual(const CC2MG &M, const C2 &L, bool norm) {
  hipStream_t st = ctx().stream;
  if (M.per[0] || M.per[1]) hipLaunchKernelGGL(kk_c2_periodic, g2(L.n0 + 2, L.n1 + 2), B2, 0, st, L, M.per[0], M.per[1]);
  if (norm) HIPCHK(hipMemsetAsync(M.d_nrm, 0, sizeof(double), st));
  hipLaunchKernelGGL(kk_c2_residual, g2(L.n0, L.n1), B2, 0, st, L, norm ? M.d_nrm : (double *)nullptr);
}
static int c2_bottom(const C2 &L) { const int N = std::max(L.n0, L.n1); return std::max(ctx().prm.mg_nub, N * N); }
static void c2_vcycle(const CC2MG &M, int l) {
  const vdn_params &P = ctx().prm;
  const C2 &L = M.lev[l];
  HIPCHK(hipMemsetAsync(L.phi, 0, sizeof(double) * c2_size(L.n0, L.n1), ctx().stream));
  if (l == (int)M.lev.size() - 1) {
    if (M.kry.w) mg_krylov_visit(M.kry, 0, P.mg_bottom_solver_eps, C2Krylov{ L, M.per[0], M.per[1], M.kry_singular }); else c2_gsrb(M, L, c2_bottom(L));
    return;
  }
  const C2 &C = M.lev[l + 1];
  c2_gsrb(M, L, P.mg_nu1);
  c2_residual(M, L, false);
  hipLaunchKernelGGL(kk_c2_restrict, g2(C.n0, C.n1), B2, 0, ctx().stream, L, C);
  c2_vcycle(M, l + 1);
  hipLaunchKernelGGL(kk_c2_prolong, g2(L.n0, L.n1), B2, 0, ctx().stream, L, C);
  c2_gsrb(M, L, P.mg_nu2);
}
int cc2_solve(CcRequest &rq) {
  vdn_multifab *rh = rq.rh, *phi = rq.phi, **beta = rq.beta; const vdn_multifab *alpha = rq.alpha;
  const double *dx = rq.dx; const int (*bc)[2] = rq.bc; const int max_iter = rq.max_iter;
  require_2d(rh, "cc_solve");
  REQUIRE(phi->ng >= 1, "cc multigrid: phi needs one ghost cell");
  hipStream_t st = ctx().stream;
  const size_t mark = arena_mark();
  const vdn_box &pd = rh->la->pd[0];
  CC2MG M; M.per[0] = bc[0][0] == VDN_BC_PER; M.per[1] = bc[1][0] == VDN_BC_PER;
  M.d_nrm = (double *)arena_alloc(256);
  int n0 = pd.hi[0] - pd.lo[0] + 1, n1 = pd.hi[1] - pd.lo[1] + 1; double h0 = dx[0], h1 = dx[1];
  long sz0 = 0;
  for (;;) {
    C2 L; L.n0 = n0; L.n1 = n1; L.P = n0 + 2; L.hi2[0] = 1.0 / (h0 * h0); L.hi2[1] = 1.0 / (h1 * h1);
    const long sz = c2_size(n0, n1);
    double *base = (double *)arena_alloc(sizeof(double) * sz * (alpha ? 6 : 5));
    HIPCHK(hipMemsetAsync(base, 0, sizeof(double) * sz * (alpha ? 6 : 5), st));
    L.phi = base; L.rh = base + sz; L.res = base + 2 * sz; L.bx = base + 3 * sz; L.by = base + 4 * sz; L.alpha = alpha ? base + 5 * sz : nullptr;
    if (M.lev.empty()) sz0 = sz * (alpha ? 6 : 5);
    M.lev.push_back(L);
    if ((n0 & 1) || (n1 & 1) || n0 <= 2 || n1 <= 2 || M.lev.size() >= 31) break;
    n0 /= 2; n1 /= 2; h0 *= 2.0; h1 *= 2.0;
  }
  // Krylov bottom solver: on the last level of a hierarchy of more than one level (a one-level hierarchy -- an odd extent on the finest level -- keeps its sweeps);
  // the statistics are those of this solve.  One workgroup below VDN_KRYLOV_GRID_MIN_POINTS_2D cells, the whole GPU from there on (krylov_grid.h), with the
  // iteration budget of this kind of bottom system (bottom_budget_begin, which reads the previous solve's statistics: before they are reset)
  const int method = mg_krylov_method(ctx().prm.mg_bottom_solver);
  if (method && M.lev.size() > 1) {
    const C2 &B = M.lev.back();
    bool dir = false;
    for (int d = 0; d < 2; d++) for (int sd = 0; sd < 2; sd++) if (bc[d][sd] == VDN_BC_DIR) dir = true;
    M.kry_singular = (!alpha && !dir) ? 1 : 0;
    GraphKey k; k.put(2); k.put(method); k.put(B.n0); k.put(B.n1); k.put(alpha ? 1 : 0); k.put(M.kry_singular); k.put(M.per); k.put(ctx().prm.mg_bottom_solver_eps);
    mg_krylov_setup(M.kry, method, c2_size(B.n0, B.n1), std::max(B.n0, B.n1), (long)B.n0 * B.n1, k, VDN_KRYLOV_GRID_MIN_POINTS_2D);
  }
  mg_krylov_begin(M.kry, 0, method != 0);
  C2Gx X; X.L = M.lev[0]; X.has_alpha = alpha ? 1 : 0;
  for (int d = 0; d < 2; d++) { X.B.lo[d] = pd.lo[d]; for (int s = 0; s < 2; s++) X.B.e[d][s] = bc[d][s]; }
  const C2 &L0 = M.lev[0];
  // level 0 of the gathered level: one launch per field over the local boxes, then (several ranks) the whole array on every rank
  std::vector<C2LoadB> vb; std::vector<C2LoadRh> vr;
  for (int b = 0; b < rh->nfabs(); b++) {
    const vdn_box &bx = rh->vbox[b];
    C2LoadB q; q.r = rng2(bx.lo[0], bx.hi[0] + (bx.hi[0] == pd.hi[0]), bx.lo[1], bx.hi[1] + (bx.hi[1] == pd.hi[1]));
    q.bxf = beta[0]->fabs[b]; q.byf = beta[1]->fabs[b]; q.af = alpha ? alpha->fabs[b] : rh->fabs[b]; q.hi[0] = bx.hi[0]; q.hi[1] = bx.hi[1];
    vb.push_back(q);
    C2LoadRh w; w.r = rng2(bx.lo[0], bx.hi[0], bx.lo[1], bx.hi[1]); w.rh = rh->fabs[b]; w.phi = phi->fabs[b];
    vr.push_back(w);
  }
  HIPCHK(hipMemsetAsync(M.d_nrm, 0, sizeof(double), st));
  launch_batched(vb, X, (double *)nullptr, 0, st);
  launch_batched(vr, X, M.d_nrm, 0, st);
  gather_level(L0.phi, sz0);
  comm_allreduce_max_dev(M.d_nrm, 1);
  for (size_t l = 1; l < M.lev.size(); l++) hipLaunchKernelGGL(kk_c2_coarsen, g2(M.lev[l].n0 + 1, M.lev[l].n1 + 1), B2, 0, st, M.lev[l - 1], M.lev[l]);
  const double bnorm = read_scalar1(M.d_nrm);
  const vdn_params &P = ctx().prm;
  int cyc = 0; bool conv = false; double rn = 0.0;
  if (bnorm == 0.0) conv = true;
  while (!conv && cyc <= max_iter) {
    c2_gsrb(M, L0, M.lev.size() == 1 ? c2_bottom(L0) : P.mg_nu1);
    c2_residual(M, L0, true);
    rn = read_scalar1(M.d_nrm);
    if (mg_converged(rn, bnorm, rq.rel_eps, rq.abs_eps)) { conv = true; break; }
    if (cyc == max_iter || !(rn < HUGE_VAL) || !(bnorm < HUGE_VAL)) break;
    if (M.lev.size() > 1) {
      hipLaunchKernelGGL(kk_c2_restrict, g2(M.lev[1].n0, M.lev[1].n1), B2, 0, st, L0, M.lev[1]);
      c2_vcycle(M, 1);
      hipLaunchKernelGGL(kk_c2_prolong, g2(L0.n0, L0.n1), B2, 0, st, L0, M.lev[1]);
      c2_gsrb(M, L0, P.mg_nu2);
    }
    cyc++;
  }
  if (M.per[0] || M.per[1]) hipLaunchKernelGGL(kk_c2_periodic, g2(L0.n0 + 2, L0.n1 + 2), B2, 0, st, L0, M.per[0], M.per[1]);
  std::vector<C2Store> vs;
  for (int b = 0; b < phi->nfabs(); b++) {
    const vdn_box &bx = phi->vbox[b];
    C2Store q; q.r = rng2(bx.lo[0] - 1, bx.hi[0] + 1, bx.lo[1] - 1, bx.hi[1] + 1); q.phi = phi->fabs[b];
    vs.push_back(q);
  }
  launch_batched(vs, X, (double *)nullptr, 0, st);
  rq.cycles = cyc; rq.res0 = bnorm; rq.res = rn;
  HIPCHK(hipStreamSynchronize(st));
  arena_release(mark);
  return conv ? 0 : 1;
}

// ---- MAC projection ---------------------------------------------------------------------------------------------------
struct divumac2_K { FV um, vm, macrhs, rh; double dxi0, dxi1;
  __device__ void cell(int i, int j, int) const {
    const double d = (G2(um, i + 1, j, 0) - G2(um, i, j, 0)) * dxi0 + (G2(vm, i, j + 1, 0) - G2(vm, i, j, 0)) * dxi1;
    P2(rh, i, j, 0) = d * -1.0 + G2(macrhs, i, j, 0);
  } };
struct mac_coeffs2_K { FV rho, bx, by; int hi0, hi1;          // hi: the box's last cell; rho is read one cell across the box's low faces (ghost-filled)
  __device__ void cell(int i, int j, int) const {
    if (j <= hi1) P2(bx, i, j, 0) = 2.0 / (G2(rho, i, j, 0) + G2(rho, i - 1, j, 0));
    if (i <= hi0) P2(by, i, j, 0) = 2.0 / (G2(rho, i, j, 0) + G2(rho, i, j - 1, 0));
  } };
struct Um2Args { int lo[2], hi[2]; int bhi[2]; double dx[2]; int ebc[2][2]; };     // lo / hi: the DOMAIN's cells (its faces carry ebc), bhi: the box's last cell
struct mkumac2_K { FV um, vm, phi, bx, by; Um2Args A;
  __device__ void cell(int i, int j, int) const {
    if (j <= A.bhi[1]) {
      const int side = (i == A.lo[0]) ? 0 : ((i == A.hi[0] + 1) ? 1 : -1);
      if (!(side >= 0 && A.ebc[0][side] == VDN_BC_NEU)) {
        const double g = (G2(phi, i, j, 0) - G2(phi, i - 1, j, 0)) / A.dx[0];
        P2(um, i, j, 0) = G2(um, i, j, 0) - G2(bx, i, j, 0) * g;
      }
    }
    if (i <= A.bhi[0]) {
      const int side = (j == A.lo[1]) ? 0 : ((j == A.hi[1] + 1) ? 1 : -1);
      if (!(side >= 0 && A.ebc[1][side] == VDN_BC_NEU)) {
        const double g = (G2(phi, i, j, 0) - G2(phi, i, j - 1, 0)) / A.dx[1];
        P2(vm, i, j, 0) = G2(vm, i, j, 0) - G2(by, i, j, 0) * g;
      }
    }
  } };
void do2_macproject(vdn_layout *mla, vdn_multifab **umac, vdn_multifab **rho, vdn_multifab **mac_rhs, const double *dx, const vdn_bc_tower *bct, int bc_comp0) {
  require_2d(rho[0], "macproject");
  const size_t mark = arena_mark();
  vdn_multifab *rh = mf_temp(mla, 0, 1, 0, -1, false, 0.0), *phi = mf_temp(mla, 0, 1, 1, -1, true, 0.0);
  vdn_multifab *beta[2] = { mf_temp(mla, 0, 1, 0, 0, false, 0.0), mf_temp(mla, 0, 1, 0, 1, false, 0.0) };
  std::vector<std::pair<divumac2_K, Range3>> vd; std::vector<std::pair<mac_coeffs2_K, Range3>> vc;
  for (int b = 0; b < rh->nfabs(); b++) {
    const vdn_box &bx = rh->vbox[b];
    vd.push_back({ divumac2_K{ umac[0]->fabs[b], umac[1]->fabs[b], mac_rhs[0]->fabs[b], rh->fabs[b], 1.0 / dx[0], 1.0 / dx[1] }, rng2(bx.lo[0], bx.hi[0], bx.lo[1], bx.hi[1]) });
    vc.push_back({ mac_coeffs2_K{ rho[0]->fabs[b], beta[0]->fabs[b], beta[1]->fabs[b], bx.hi[0], bx.hi[1] }, rng2(bx.lo[0], bx.hi[0] + 1, bx.lo[1], bx.hi[1] + 1) });
  }
  run_cells(vd); run_cells(vc);
  int ebc[3][2];
  for (int d = 0; d < 3; d++) for (int s = 0; s < 2; s++) ebc[d][s] = d < 2 ? bct->ell_bc(0, 0, d, s, bc_comp0) : VDN_BC_INT;
  CcRequest q;
  q.rh = rh; q.phi = phi; q.beta = beta; q.dx = dx; q.bc = ebc; q.rel_eps = ctx().prm.mac_rel_eps; q.max_iter = ctx().prm.mg_max_iter;
  const int rc = cc2_solve(q);
  ctx().solver_cycles[0] = q.cycles; ctx().solver_res0[0] = q.res0; ctx().solver_res[0] = q.res;
  solver_check(rc, "MAC multigrid (2-D)", q.cycles, q.res, q.res0);
  // (phi's ghost layer came from the gathered solve: the neighbours' phi across a box face, the closure across a domain face)
  const vdn_box &pd = mla->pd[0];
  std::vector<std::pair<mkumac2_K, Range3>> vu;
  for (int b = 0; b < rh->nfabs(); b++) {
    const vdn_box &bx = rh->vbox[b];
    Um2Args A;
    for (int d = 0; d < 2; d++) { A.lo[d] = pd.lo[d]; A.hi[d] = pd.hi[d]; A.bhi[d] = bx.hi[d]; A.dx[d] = dx[d]; for (int s = 0; s < 2; s++) A.ebc[d][s] = ebc[d][s]; }
    vu.push_back({ mkumac2_K{ umac[0]->fabs[b], umac[1]->fabs[b], phi->fabs[b], beta[0]->fabs[b], beta[1]->fabs[b], A }, rng2(bx.lo[0], bx.hi[0] + 1, bx.lo[1], bx.hi[1] + 1) });
  }
  run_cells(vu);
  mf_fill_boundary(umac[0]); mf_fill_boundary(umac[1]);
  mf_temp_free(beta[0]); mf_temp_free(beta[1]); mf_temp_free(phi); mf_temp_free(rh);
  arena_release(mark);
}

// ---- explicit diffusive term and the implicit viscous / diffusive solves ------------------------------------------------
struct Lap2Args { int lo[2], hi[2]; int e[2][2]; double hi2[2]; int comp; };
struct lap2_K { FV lap, data; Lap2Args A;          // A: the box and its own boundary codes (interior faces: no folding)
  __device__ void cell(int i, int j, int) const {
    const int q[2] = { i, j };
    const double p0 = G2(data, i, j, A.comp);
    double sum = 0.0;
    #pragma unroll
    for (int d = 0; d < 2; d++) {
      const int mi = i - (d == 0), mj = j - (d == 1), pi = i + (d == 0), pj = j + (d == 1);
      double fm = p0 - G2(data, mi, mj, A.comp), fp = G2(data, pi, pj, A.comp) - p0;
      if (q[d] == A.lo[d]) { if (A.e[d][0] == VDN_BC_NEU) fm = 0.0; else if (A.e[d][0] == VDN_BC_DIR) fm = 2.0 * fm; }
      if (q[d] == A.hi[d]) { if (A.e[d][1] == VDN_BC_NEU) fp = 0.0; else if (A.e[d][1] == VDN_BC_DIR) fp = 2.0 * fp; }
      sum = sum + (fp - fm) * A.hi2[d];
    }
    P2(lap, i, j, A.comp) = sum;
  } };
void k2_explicit_diffusive_term(vdn_multifab *lap, const vdn_multifab *data, int comp, int bccomp0, const double *dx, const vdn_bc_tower *bct) {
  std::vector<std::pair<lap2_K, Range3>> v;
  for (int b = 0; b < lap->nfabs(); b++) {
    Lap2Args A; const vdn_box &bx = lap->vbox[b];
    for (int d = 0; d < 2; d++) { A.lo[d] = bx.lo[d]; A.hi[d] = bx.hi[d]; A.hi2[d] = 1.0 / (dx[d] * dx[d]); for (int s = 0; s < 2; s++) A.e[d][s] = bct->ell_bc(lap->lev, b + 1, d, s, bccomp0); }
    A.comp = comp;
    v.push_back({ lap2_K{ lap->fabs[b], data->fabs[b], A }, rng2(bx.lo[0], bx.hi[0], bx.lo[1], bx.hi[1]) });
  }
  run_cells(v);
}
struct Vr2Args { int d, dtype; double mu, third_mudt, dxd; int lo[2], hi[2]; };
struct visc_rhs2_K { FV rh, phi, unew, rho, lapu, macrhs; Vr2Args A;
  __device__ void cell(int i, int j, int) const {      // range = valid box grown by 1: phi takes unew incl. the ghost layer
    P2(phi, i, j, 0) = G2(unew, i, j, A.d);
    if (i < A.lo[0] || i > A.hi[0] || j < A.lo[1] || j > A.hi[1]) return;
    double r = G2(unew, i, j, A.d) * G2(rho, i, j, 0);
    if (A.dtype == 1) r = r + A.mu * G2(lapu, i, j, A.d);
    const int pi = i + (A.d == 0), pj = j + (A.d == 1), mi = i - (A.d == 0), mj = j - (A.d == 1);
    r = r + A.third_mudt * (G2(macrhs, pi, pj, 0) - G2(macrhs, mi, mj, 0)) / A.dxd;
    P2(rh, i, j, 0) = r;
  } };
struct diff_rhs2_K { FV rh, phi, snew, laps; int comp, dtype; double mu; int lo[2], hi[2];
  __device__ void cell(int i, int j, int) const {
    P2(phi, i, j, 0) = G2(snew, i, j, comp);
    if (i < lo[0] || i > hi[0] || j < lo[1] || j > hi[1]) return;
    double r = G2(snew, i, j, comp);
    if (dtype == 1) r = r + mu * G2(laps, i, j, comp);
    P2(rh, i, j, 0) = r;
  } };
void do2_visc_solve(vdn_layout *mla, vdn_multifab *unew, const vdn_multifab *lapu, const vdn_multifab *rho, const vdn_multifab *mac_rhs,
                    const double *dx, double mu, const vdn_bc_tower *bct) {
  require_2d(unew, "visc_solve");
  const size_t mark = arena_mark();
  vdn_multifab *rh = mf_temp(mla, 0, 1, 0, -1, false, 0.0), *phi = mf_temp(mla, 0, 1, 1, -1, true, 0.0), *alpha = mf_temp(mla, 0, 1, 0, -1, false, 0.0);
  vdn_multifab *beta[2] = { mf_temp(mla, 0, 1, 0, 0, true, mu), mf_temp(mla, 0, 1, 0, 1, true, mu) };
  mf_copy(alpha, 0, rho, 0, 1, 0);
  const int dtype = ctx().prm.diffusion_type;
  for (int d = 0; d < 2; d++) {
    std::vector<std::pair<visc_rhs2_K, Range3>> v;
    for (int b = 0; b < unew->nfabs(); b++) {
      const vdn_box &bx = unew->vbox[b];
      Vr2Args A; A.d = d; A.dtype = dtype; A.mu = mu; A.third_mudt = (1.0 / 3.0) * ((dtype == 1) ? 2.0 * mu : mu); A.dxd = dx[d];
      for (int a = 0; a < 2; a++) { A.lo[a] = bx.lo[a]; A.hi[a] = bx.hi[a]; }
      v.push_back({ visc_rhs2_K{ rh->fabs[b], phi->fabs[b], unew->fabs[b], rho->fabs[b], lapu ? lapu->fabs[b] : unew->fabs[b], mac_rhs->fabs[b], A },
                    rng2(bx.lo[0] - 1, bx.hi[0] + 1, bx.lo[1] - 1, bx.hi[1] + 1) });
    }
    run_cells(v);
    int ebc[3][2];
    for (int a = 0; a < 3; a++) for (int s = 0; s < 2; s++) ebc[a][s] = a < 2 ? bct->ell_bc(0, 0, a, s, d) : VDN_BC_INT;
    CcRequest q;
    q.rh = rh; q.phi = phi; q.beta = beta; q.alpha = alpha; q.dx = dx; q.bc = ebc; q.rel_eps = 1.e-12; q.max_iter = ctx().prm.mg_max_iter;
    const int rc = cc2_solve(q);
    solver_check(rc, "viscous solve (2-D)", q.cycles, q.res, q.res0, d);
    mf_copy(unew, d, phi, 0, 1, 0);
  }
  mf_restrict_and_fill(unew, 0, 0, 2, false, bct);
  mf_temp_free(beta[0]); mf_temp_free(beta[1]); mf_temp_free(alpha); mf_temp_free(phi); mf_temp_free(rh);
  arena_release(mark);
}
void do2_diff_scalar_solve(vdn_layout *mla, vdn_multifab *snew, const vdn_multifab *laps, const double *dx, double mu, const vdn_bc_tower *bct, int icomp, int bccomp0) {
  require_2d(snew, "diff_scalar_solve");
  const size_t mark = arena_mark();
  vdn_multifab *rh = mf_temp(mla, 0, 1, 0, -1, false, 0.0), *phi = mf_temp(mla, 0, 1, 1, -1, true, 0.0), *alpha = mf_temp(mla, 0, 1, 0, -1, true, 1.0);
  vdn_multifab *beta[2] = { mf_temp(mla, 0, 1, 0, 0, true, mu), mf_temp(mla, 0, 1, 0, 1, true, mu) };
  std::vector<std::pair<diff_rhs2_K, Range3>> v;
  for (int b = 0; b < snew->nfabs(); b++) {
    const vdn_box &bx = snew->vbox[b];
    v.push_back({ diff_rhs2_K{ rh->fabs[b], phi->fabs[b], snew->fabs[b], laps ? laps->fabs[b] : snew->fabs[b], icomp, ctx().prm.diffusion_type, mu,
                               { bx.lo[0], bx.lo[1] }, { bx.hi[0], bx.hi[1] } },
                  rng2(bx.lo[0] - 1, bx.hi[0] + 1, bx.lo[1] - 1, bx.hi[1] + 1) });
  }
  run_cells(v);
  int ebc[3][2];
  for (int a = 0; a < 3; a++) for (int s = 0; s < 2; s++) ebc[a][s] = a < 2 ? bct->ell_bc(0, 0, a, s, bccomp0) : VDN_BC_INT;
  CcRequest q;
  q.rh = rh; q.phi = phi; q.beta = beta; q.alpha = alpha; q.dx = dx; q.bc = ebc; q.rel_eps = 1.e-12; q.max_iter = ctx().prm.mg_max_iter;
  const int rc = cc2_solve(q);
  solver_check(rc, "diffusive solve (2-D)", q.cycles, q.res, q.res0);
  mf_copy(snew, icomp, phi, 0, 1, 0);
  mf_restrict_and_fill(snew, icomp, bccomp0, 1, false, bct);
  mf_temp_free(beta[0]); mf_temp_free(beta[1]); mf_temp_free(alpha); mf_temp_free(phi); mf_temp_free(rh);
  arena_release(mark);
}

// =====================================================================================================================
// nodal multigrid, 9-point Q1:  K phi = b,  b = -rh
// =====================================================================================================================
struct N2 { int n0, n1, PN, PS; double f[2]; double *phi, *tmp, *b, *res, *sig; int dirlo[2], dirhi[2]; };
KRY_HD long n2_nsize(int n0, int n1) { return (long)(n0 + 3) * (n1 + 3); }
DEVI long n2i(const N2 &L, int i, int j) { return (long)(i + 1) + (long)L.PN * (j + 1); }
DEVI long s2i(const N2 &L, int i, int j) { return (long)(i + 1) + (long)L.PS * (j + 1); }
DEVI bool n2_dir(const N2 &L, int i, int j) {
  return (i == 0 && L.dirlo[0]) || (i == L.n0 && L.dirhi[0]) || (j == 0 && L.dirlo[1]) || (j == L.n1 && L.dirhi[1]);
}
// cells (cj,ci) ascending, corners (my,mx) ascending -- the order of nd_apply's dm = 2 branch in oracle/vo_hgproject.c
DEVI void n2_apply(const N2 &L, const double *__restrict__ phi, int i, int j, double &Kp, double &diag) {
  const double fx = L.f[0], fy = L.f[1];
  double w[4];
  w[0] = 2.0 * (fx + fy); w[1] = -2.0 * fx + fy; w[2] = fx - 2.0 * fy; w[3] = -(fx + fy);
  double acc = 0.0, ssum = 0.0;
  #pragma unroll
  for (int dj = 0; dj < 2; dj++)
    #pragma unroll
    for (int di = 0; di < 2; di++) {
      const int ci = i - 1 + di, cj = j - 1 + dj;
      const double sg = L.sig[s2i(L, ci, cj)];
      double t = 0.0;
      #pragma unroll
      for (int my = 0; my < 2; my++)
        #pragma unroll
        for (int mx = 0; mx < 2; mx++) {
          const int ni = ci + mx, nj = cj + my;
          const int idx = (ni != i) | ((nj != j) << 1);
          t = t + w[idx] * phi[n2i(L, ni, nj)];
        }
      acc = acc + sg * t;
      ssum = ssum + sg;
    }
  Kp = acc; diag = w[0] * ssum;
}
// entry (i, j) of the node array grown by one: the image along a periodic direction, zero on the ring beyond a physical face (the source is a node no thread
// writes: below n along a periodic direction, on the level along the other)
DEVI void n2_fill_entry(const N2 &L, double *a, int per0, int per1, int i, int j) {
  int si = i, sj = j; bool g = false, zero = false;
  if (per0) { if (i < 0) { si = i + L.n0; g = true; } else if (i >= L.n0) { si = i - L.n0; g = true; } } else if (i < 0 || i > L.n0) { g = true; zero = true; }
  if (per1) { if (j < 0) { sj = j + L.n1; g = true; } else if (j >= L.n1) { sj = j - L.n1; g = true; } } else if (j < 0 || j > L.n1) { g = true; zero = true; }
  if (g) a[n2i(L, i, j)] = zero ? 0.0 : a[n2i(L, si, sj)];
}
__global__ void kk_n2_fill_nodes(N2 L, double *a, int per0, int per1) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x) - 1, j = (int)(blockIdx.y * blockDim.y + threadIdx.y) - 1;
  if (i > L.n0 + 1 || j > L.n1 + 1) return;
  n2_fill_entry(L, a, per0, per1, i, j);
}
__global__ void kk_n2_fill_cells(N2 L, int per0, int per1) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x) - 1, j = (int)(blockIdx.y * blockDim.y + threadIdx.y) - 1;
  if (i > L.n0 || j > L.n1) return;
  int si = i, sj = j; bool g = false, zero = false;
  if (i < 0) { g = true; if (per0) si = i + L.n0; else zero = true; } else if (i >= L.n0) { g = true; if (per0) si = i - L.n0; else zero = true; }
  if (j < 0) { g = true; if (per1) sj = j + L.n1; else zero = true; } else if (j >= L.n1) { g = true; if (per1) sj = j - L.n1; else zero = true; }
  if (g) L.sig[s2i(L, i, j)] = zero ? 0.0 : L.sig[s2i(L, si, sj)];
}
__global__ void kk_n2_jacobi(N2 L, const double *__restrict__ phi, double *__restrict__ out, double omega) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i > L.n0 || j > L.n1) return;
  const long c = n2i(L, i, j);
  const double p0 = phi[c];
  double v = p0;
  if (!n2_dir(L, i, j)) { double Kp, diag; n2_apply(L, phi, i, j, Kp, diag); if (diag != 0.0) v = p0 + omega * ((L.b[c] - Kp) / diag); }
  out[c] = v;
}
__global__ void kk_n2_residual(N2 L, double *nrm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  double r = 0.0;
  if (i <= L.n0 && j <= L.n1) {
    if (!n2_dir(L, i, j)) { double Kp, diag; n2_apply(L, L.phi, i, j, Kp, diag); r = L.b[n2i(L, i, j)] - Kp; }
    L.res[n2i(L, i, j)] = r;
  }
  if (nrm) block_atomic_max(nrm, fabs(r));
}
__global__ void kk_n2_restrict(N2 F, N2 C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i > C.n0 || j > C.n1) return;
  const double wt[3] = { 0.5, 1.0, 0.5 };
  double s = 0.0;
  if (!n2_dir(C, i, j))
    for (int b = -1; b <= 1; b++) for (int a = -1; a <= 1; a++) s = s + (wt[a + 1] * wt[b + 1]) * F.res[n2i(F, 2 * i + a, 2 * j + b)];
  C.b[n2i(C, i, j)] = s * 0.25;
}
__global__ void kk_n2_prolong(N2 F, N2 C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i > F.n0 || j > F.n1 || n2_dir(F, i, j)) return;
  const int I = i >> 1, J = j >> 1, oi = i & 1, oj = j & 1;
  double s = 0.0;
  for (int b = 0; b <= oj; b++) for (int a = 0; a <= oi; a++) s = s + C.phi[n2i(C, I + a, J + b)];
  const double scale = 1.0 / (double)((1 + oi) * (1 + oj));
  F.phi[n2i(F, i, j)] = F.phi[n2i(F, i, j)] + s * scale;
}
__global__ void kk_n2_coarsen_sigma(N2 F, N2 C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
  if (i >= C.n0 || j >= C.n1) return;
  double s = 0.0;
  for (int b = 0; b < 2; b++) for (int a = 0; a < 2; a++) s = s + F.sig[s2i(F, 2 * i + a, 2 * j + b)];
  C.sig[s2i(C, i, j)] = s * 0.25;
}
// ---- Krylov bottom solver (vdn_params.hg_bottom_solver = 1, 2, 3; krylov_wg.h) -- the 2-D counterpart of mg_nd.hip's NdKrylov ----
// The 26^2-node bottom of a 200^2 problem takes max(hg_nub, 2 N^2) = 1250 Jacobi sweeps of two launches each.  K as n2_apply returns it is symmetric positive
// semi-definite with a positive diagonal.  Dirichlet (outflow) nodes are not unknowns; along a periodic direction node n is the image of node 0, written by the
// fill only and counted once.  The sigma = 0 ring beyond a physical face is the wall closure and the node ring there reads as zero (the fill writes it).  The
// solve starts from phi = 0 and leaves its result in the array L.phi names at the launch (no ping-pong: the host's phi / tmp swap is that of zero sweeps).
// ... one entry of the padded array at a time (kg_fill of the grid-wide form, krylov_grid.h; wg_n2_fill_nodes).  Without a periodic direction the grid-wide form has nothing
// to do: every written entry would be a zero of the ring, which the visit's memsets (the work arrays) and the V-cycle's (phi) have left zero and no kernel of the solve writes.
KRY_HD int n2_fill_count(const N2 &L, int per0, int per1) { return (per0 || per1) ? (L.n0 + 3) * (L.n1 + 3) : 0; }
DEVI void n2_fill_point(const N2 &L, double *a, int per0, int per1, int t) { const int nx = L.n0 + 3; n2_fill_entry(L, a, per0, per1, t % nx - 1, t / nx - 1); }
DEVI void wg_n2_fill_nodes(const N2 &L, double *a, int per0, int per1) {      // kk_n2_fill_nodes by one workgroup (the zero ring included, whatever is periodic); ends in a barrier
  const int np = (L.n0 + 3) * (L.n1 + 3);
  for (int t = threadIdx.x; t < np; t += blockDim.x) n2_fill_point(L, a, per0, per1, t);
  __syncthreads();
}
// the level as wg_krylov, the grid-wide kernels and the host (mg_krylov_visit) take it (krylov_wg.h): by value -- L.phi is the array the level's phi names at the visit
struct N2Krylov {
  N2 L; int per0, per1;
  KRY_HD int count() const { return (L.n0 + 1) * (L.n1 + 1); }
  DEVI bool point(int t, long &c, int &i, int &j, int &k) const {
    const int nx = L.n0 + 1;
    i = t % nx; j = t / nx; k = 0; c = n2i(L, i, j);
    return !n2_dir(L, i, j) && !((per0 && i == L.n0) || (per1 && j == L.n1));
  }
  DEVI void apply(const double *v, long, int i, int j, int, double &Av, double &diag) const { n2_apply(L, v, i, j, Av, diag); }
  DEVI void fill(double *v) const { wg_n2_fill_nodes(L, v, per0, per1); }
  KRY_HD int fill_count() const { return n2_fill_count(L, per0, per1); }
  DEVI void fill_point(double *v, int t) const { n2_fill_point(L, v, per0, per1, t); }
  KRY_HD long size() const { return n2_nsize(L.n0, L.n1); }
  DEVI const double *rhs() const { return L.b; }
  DEVI double *x() const { return L.phi; }
  KRY_HD bool singular() const { return !(L.dirlo[0] || L.dirlo[1] || L.dirhi[0] || L.dirhi[1]); }
};
struct N2Gx { N2 L; int lo[2]; };                      // lo: the domain's first cell / node
// gathered level (see cc2_solve): sigma on the box's cells, grown by the ghost cell at the domain's sides (the ring the smoother reads there)
struct N2LoadSig { Range3 r; int g[3]; FV coeffs;
  static __device__ double body(const N2LoadSig &q, int gi, int gj, int, const N2Gx &x) {
    x.L.sig[s2i(x.L, gi - x.lo[0], gj - x.lo[1])] = G2(q.coeffs, gi, gj, 0);
    return 0.0;
  } };
// b = -rh and phi on the box's nodes, grown by the high nodes at the domain's high sides (a node that boxes share comes from the box that
// holds the cell on its high side along both directions); returns |rh| for the norm
struct N2Load { Range3 r; int g[3]; FV rh, phi;
  static __device__ double body(const N2Load &q, int gi, int gj, int, const N2Gx &x) {
    const N2 &L = x.L;
    const int i = gi - x.lo[0], j = gj - x.lo[1];
    const bool dir = n2_dir(L, i, j);
    const double r = dir ? 0.0 : G2(q.rh, gi, gj, 0);
    L.b[n2i(L, i, j)] = -r;
    L.phi[n2i(L, i, j)] = dir ? 0.0 : G2(q.phi, gi, gj, 0);
    return fabs(r);
  } };
// phi back on every node of the box's fab, ghost layer included (the domain array's ghost ring holds the periodic images / zeros)
struct N2Store { Range3 r; int g[3]; FV phi;
  static __device__ double body(const N2Store &q, int gi, int gj, int, const N2Gx &x) {
    P2(q.phi, gi, gj, 0) = x.L.phi[n2i(x.L, gi - x.lo[0], gj - x.lo[1])];
    return 0.0;
  } };
struct nd_divu2_K { FV u, rh; double gx, gy;
  __device__ void cell(int i, int j, int) const {
    const double dux = (G2(u, i, j, 0) + G2(u, i, j - 1, 0)) - (G2(u, i - 1, j, 0) + G2(u, i - 1, j - 1, 0));
    const double duy = (G2(u, i, j, 1) + G2(u, i - 1, j, 1)) - (G2(u, i, j - 1, 1) + G2(u, i - 1, j - 1, 1));
    P2(rh, i, j, 0) = G2(rh, i, j, 0) + (dux * gx + duy * gy);
  } };
struct ND2MG { std::vector<N2> lev; int per[2]; double *d_nrm;
  MgKrylov kry; };      // Krylov bottom solver (kry.w == nullptr: the bottom sweeps; kry.part: the grid-wide form)
static void n2_fill(const ND2MG &M, const N2 &L, double *a) { hipLaunchKernelGGL(kk_n2_fill_nodes, g2(L.n0 + 3, L.n1 + 3), B2, 0, ctx().stream, L, a, M.per[0], M.per[1]); }
static void n2_jacobi(const ND2MG &M, N2 &L, int ns) {
  for (int s = 0; s < ns; s++) {
    n2_fill(M, L, L.phi);
    hipLaunchKernelGGL(kk_n2_jacobi, g2(L.n0 + 1, L.n1 + 1), B2, 0, ctx().stream, L, (const double *)L.phi, L.tmp, ctx().prm.hg_omega);
    std::swap(L.phi, L.tmp);
  }
}
static void n2_residual(const ND2MG &M, N2 &L, bool norm) {
  n2_fill(M, L, L.phi);
  if (norm) HIPCHK(hipMemsetAsync(M.d_nrm, 0, sizeof(double), ctx().stream));
  hipLaunchKernelGGL(kk_n2_residual, g2(L.n0 + 1, L.n1 + 1), B2, 0, ctx().stream, L, norm ? M.d_nrm : (double *)nullptr);
  n2_fill(M, L, L.res);
}
static int n2_bottom(const N2 &L) { const int N = std::max(L.n0, L.n1); return std::max(ctx().prm.hg_nub, 2 * N * N); }
static void n2_vcycle(ND2MG &M, int l) {
  const vdn_params &P = ctx().prm;
  N2 &L = M.lev[l];
  HIPCHK(hipMemsetAsync(L.phi, 0, sizeof(double) * n2_nsize(L.n0, L.n1), ctx().stream));
  if (l == (int)M.lev.size() - 1) {
    // (the result is left in the array L.phi names now: the sweeps above this level may have swapped phi and tmp, the Krylov solve swaps nothing)
    if (M.kry.w) mg_krylov_visit(M.kry, 1, P.hg_bottom_solver_eps, N2Krylov{ L, M.per[0], M.per[1] }); else n2_jacobi(M, L, n2_bottom(L));
    return;
  }
  N2 &C = M.lev[l + 1];
  n2_jacobi(M, L, P.hg_nu1);
  n2_residual(M, L, false);
  hipLaunchKernelGGL(kk_n2_restrict, g2(C.n0 + 1, C.n1 + 1), B2, 0, ctx().stream, L, C);
  n2_vcycle(M, l + 1);
  n2_fill(M, C, C.phi);
  hipLaunchKernelGGL(kk_n2_prolong, g2(L.n0 + 1, L.n1 + 1), B2, 0, ctx().stream, L, C);
  n2_jacobi(M, L, P.hg_nu2);
}
int nd2_solve(NdRequest &rq) {
  vdn_multifab *rh = rq.rh, *phi = rq.phi; const vdn_multifab *coeffs = rq.coeffs, *u = rq.u;
  const double *dx = rq.dx; const int (*bc)[2] = rq.bc; const int max_iter = rq.max_iter;
  require_2d(coeffs, "nd_solve");
  REQUIRE(phi->ng >= 1 && rh->ng >= 1 && coeffs->ng >= 1, "nodal multigrid: phi, rh, coeffs need one ghost layer");
  hipStream_t st = ctx().stream;
  const size_t mark = arena_mark();
  const vdn_box &pd = coeffs->la->pd[0];
  ND2MG M; M.per[0] = coeffs->la->pmask[0]; M.per[1] = coeffs->la->pmask[1];
  M.d_nrm = (double *)arena_alloc(256);
  int n0 = pd.hi[0] - pd.lo[0] + 1, n1 = pd.hi[1] - pd.lo[1] + 1; double h0 = dx[0], h1 = dx[1];
  long sz0 = 0;
  for (;;) {
    N2 L; L.n0 = n0; L.n1 = n1; L.PN = n0 + 3; L.PS = n0 + 2; L.f[0] = 1.0 / (6.0 * (h0 * h0)); L.f[1] = 1.0 / (6.0 * (h1 * h1));
    for (int d = 0; d < 2; d++) { L.dirlo[d] = bc[d][0] == VDN_BC_DIR; L.dirhi[d] = bc[d][1] == VDN_BC_DIR; }
    const long nn = n2_nsize(n0, n1), ns = (long)(n0 + 2) * (n1 + 2);
    double *base = (double *)arena_alloc(sizeof(double) * (4 * nn + ns));
    HIPCHK(hipMemsetAsync(base, 0, sizeof(double) * (4 * nn + ns), st));
    L.phi = base; L.tmp = base + nn; L.b = base + 2 * nn; L.res = base + 3 * nn; L.sig = base + 4 * nn;
    if (M.lev.empty()) sz0 = 4 * nn + ns;
    M.lev.push_back(L);
    if ((n0 & 1) || (n1 & 1) || n0 <= 2 || n1 <= 2 || M.lev.size() >= 31) break;
    n0 /= 2; n1 /= 2; h0 *= 2.0; h1 *= 2.0;
  }
  // Krylov bottom solver: as in cc2_solve (more than one level; the statistics are those of this solve)
  const int method = mg_krylov_method(ctx().prm.hg_bottom_solver);
  if (method && M.lev.size() > 1) {
    const N2 &B = M.lev.back();
    GraphKey k; k.put(3); k.put(method); k.put(B.n0); k.put(B.n1); k.put(B.dirlo); k.put(B.dirhi); k.put(M.per); k.put(ctx().prm.hg_bottom_solver_eps);
    mg_krylov_setup(M.kry, method, n2_nsize(B.n0, B.n1), std::max(B.n0, B.n1) + 1, (long)(B.n0 + 1) * (B.n1 + 1), k, VDN_KRYLOV_GRID_MIN_POINTS_2D);
  }
  mg_krylov_begin(M.kry, 1, method != 0);
  N2 &L0 = M.lev[0];
  N2Gx X; X.L = L0; X.lo[0] = pd.lo[0]; X.lo[1] = pd.lo[1];
  if (u) {
    std::vector<std::pair<nd_divu2_K, Range3>> v;
    for (int b = 0; b < rh->nfabs(); b++) {
      const vdn_box &bx = rh->vbox[b];
      v.push_back({ nd_divu2_K{ u->fabs[b], rh->fabs[b], 0.5 / dx[0], 0.5 / dx[1] }, rng2(bx.lo[0], bx.hi[0] + 1, bx.lo[1], bx.hi[1] + 1) });
    }
    run_cells(v);
  }
  // level 0 of the gathered level: one launch per field over the local boxes, then (several ranks) the whole array on every rank
  std::vector<N2LoadSig> vs; std::vector<N2Load> vl;
  for (int b = 0; b < coeffs->nfabs(); b++) {
    const vdn_box &bx = coeffs->vbox[b];
    const int alo[2] = { bx.lo[0] == pd.lo[0], bx.lo[1] == pd.lo[1] }, ahi[2] = { bx.hi[0] == pd.hi[0], bx.hi[1] == pd.hi[1] };
    N2LoadSig q; q.r = rng2(bx.lo[0] - alo[0], bx.hi[0] + ahi[0], bx.lo[1] - alo[1], bx.hi[1] + ahi[1]); q.coeffs = coeffs->fabs[b];
    vs.push_back(q);
    N2Load w; w.r = rng2(bx.lo[0], bx.hi[0] + ahi[0], bx.lo[1], bx.hi[1] + ahi[1]); w.rh = rh->fabs[b]; w.phi = phi->fabs[b];
    vl.push_back(w);
  }
  HIPCHK(hipMemsetAsync(M.d_nrm, 0, sizeof(double), st));
  launch_batched(vs, X, (double *)nullptr, 0, st);
  launch_batched(vl, X, M.d_nrm, 0, st);
  gather_level(L0.phi, sz0);
  comm_allreduce_max_dev(M.d_nrm, 1);
  for (size_t l = 1; l < M.lev.size(); l++) {
    hipLaunchKernelGGL(kk_n2_coarsen_sigma, g2(M.lev[l].n0, M.lev[l].n1), B2, 0, st, M.lev[l - 1], M.lev[l]);
    hipLaunchKernelGGL(kk_n2_fill_cells, g2(M.lev[l].n0 + 2, M.lev[l].n1 + 2), B2, 0, st, M.lev[l], M.per[0], M.per[1]);
  }
  const double bnorm = read_scalar1(M.d_nrm);
  const vdn_params &P = ctx().prm;
  int cyc = 0; bool conv = (bnorm == 0.0); double rn = 0.0;
  while (!conv) {
    n2_jacobi(M, L0, M.lev.size() == 1 ? n2_bottom(L0) : P.hg_nu1);
    n2_residual(M, L0, true);
    rn = read_scalar1(M.d_nrm);
    if (mg_converged(rn, bnorm, rq.rel_eps, rq.abs_eps)) { conv = true; break; }
    if (cyc >= max_iter || !(rn < HUGE_VAL) || !(bnorm < HUGE_VAL)) break;     // also: a NaN / inf norm (the reductions turn NaN into +inf)
    if (M.lev.size() > 1) {
      hipLaunchKernelGGL(kk_n2_restrict, g2(M.lev[1].n0 + 1, M.lev[1].n1 + 1), B2, 0, st, L0, M.lev[1]);
      n2_vcycle(M, 1);
      n2_fill(M, M.lev[1], M.lev[1].phi);
      hipLaunchKernelGGL(kk_n2_prolong, g2(L0.n0 + 1, L0.n1 + 1), B2, 0, st, L0, M.lev[1]);
      n2_jacobi(M, L0, P.hg_nu2);
    }
    cyc++;
  }
  n2_fill(M, L0, L0.phi);
  X.L = L0;                                          // (the smoother swaps phi and tmp)
  std::vector<N2Store> vo;
  for (int b = 0; b < phi->nfabs(); b++) {
    const vdn_box &bx = phi->vbox[b];
    N2Store q; q.r = rng2(bx.lo[0] - 1, bx.hi[0] + 2, bx.lo[1] - 1, bx.hi[1] + 2); q.phi = phi->fabs[b];
    vo.push_back(q);
  }
  launch_batched(vo, X, (double *)nullptr, 0, st);
  rq.cycles = cyc; rq.res0 = bnorm; rq.res = rn;
  HIPCHK(hipStreamSynchronize(st));
  arena_release(mark);
  return conv ? 0 : 1;
}

// ---- HG projection ------------------------------------------------------------------------------------------------------
struct Uv2Args { int lo[2], hi[2]; int phys[2][2]; int proj_type; double dt, dtinv; };     // the box and its own physical boundary codes
struct create_uvec2_K { FV unew, uold, rhohalf, gp; Uv2Args A;
  __device__ void cell(int i, int j, int) const {      // range = box grown by the ghost width of unew
    const int q[2] = { i, j };
    bool g1 = true, wall_plane = false, inlet_plane = false;
    #pragma unroll
    for (int d = 0; d < 2; d++) {
      if (q[d] < A.lo[d] - 1 || q[d] > A.hi[d] + 1) g1 = false;
      if (q[d] == A.lo[d] - 1) { const int p = A.phys[d][0]; if (p == VDN_SLIP_WALL || p == VDN_NO_SLIP_WALL) wall_plane = true; if (p == VDN_INLET) inlet_plane = true; }
      if (q[d] == A.hi[d] + 1) { const int p = A.phys[d][1]; if (p == VDN_SLIP_WALL || p == VDN_NO_SLIP_WALL) wall_plane = true; if (p == VDN_INLET) inlet_plane = true; }
    }
    #pragma unroll
    for (int m = 0; m < 2; m++) {
      double gpv = 0.0;
      if (g1) { gpv = G2(gp, i, j, m); if (inlet_plane) { gpv = 0.0; P2(gp, i, j, m) = 0.0; } }
      if (wall_plane) { P2(unew, i, j, m) = 0.0; continue; }
      if (!g1) continue;
      double v = G2(unew, i, j, m);
      if (A.proj_type == VDN_PRESSURE_ITERS) v = (v - G2(uold, i, j, m)) * A.dtinv;
      else if (A.proj_type == VDN_REGULAR_TIMESTEP) v = v + A.dt * gpv / G2(rhohalf, i, j, 0);
      P2(unew, i, j, m) = v;
    }
  } };
struct coeffs2_K { FV coeffs, rhohalf;
  __device__ void cell(int i, int j, int) const { P2(coeffs, i, j, 0) = 1.0 / G2(rhohalf, i, j, 0); } };
struct Hg2Args { int hi[2]; double dt, dtinv, dxi[2]; int proj_type; };
struct hg_update2_K { FV unew, uold, gp, rhohalf, p, phi; Hg2Args A;
  __device__ void cell(int i, int j, int) const {      // range = the box's nodes lo..hi+1
    if (i <= A.hi[0] && j <= A.hi[1]) {
      const double gph[2] = { 0.5 * (G2(phi, i + 1, j, 0) + G2(phi, i + 1, j + 1, 0) - G2(phi, i, j, 0) - G2(phi, i, j + 1, 0)) * A.dxi[0],      // mkgphi_2d
                              0.5 * (G2(phi, i, j + 1, 0) + G2(phi, i + 1, j + 1, 0) - G2(phi, i, j, 0) - G2(phi, i + 1, j, 0)) * A.dxi[1] };
      const double rho = G2(rhohalf, i, j, 0);
      #pragma unroll
      for (int m = 0; m < 2; m++) {
        double v = G2(unew, i, j, m) - gph[m] / rho;
        if (A.proj_type == VDN_PRESSURE_ITERS) v = G2(uold, i, j, m) + A.dt * v;
        P2(unew, i, j, m) = v;
        if (A.proj_type == VDN_PRESSURE_ITERS) P2(gp, i, j, m) = G2(gp, i, j, m) + gph[m];
        else if (A.proj_type == VDN_REGULAR_TIMESTEP) P2(gp, i, j, m) = A.dtinv * gph[m];
      }
    }
    if (A.proj_type == VDN_PRESSURE_ITERS) P2(p, i, j, 0) = G2(p, i, j, 0) + G2(phi, i, j, 0);
    else if (A.proj_type == VDN_REGULAR_TIMESTEP) P2(p, i, j, 0) = A.dtinv * G2(phi, i, j, 0);
  } };
void do2_hgproject(int proj_type, vdn_layout *mla, vdn_multifab **unew, vdn_multifab **uold, vdn_multifab **rhohalf, vdn_multifab **p, vdn_multifab **gp,
                   const double *dx, double dt, const vdn_bc_tower *bct, int press_comp0) {
  vdn_multifab *un = unew[0], *uo = uold[0], *rhh = rhohalf[0], *pp = p[0], *gpp = gp[0];
  require_2d(un, "hgproject");
  const size_t mark = arena_mark();
  vdn_multifab *rh = mf_temp(mla, 0, 1, 1, 3, true, 0.0), *phi = mf_temp(mla, 0, 1, 1, 3, true, 0.0), *coeffs = mf_temp(mla, 0, 1, 1, -1, true, 0.0);
  std::vector<std::pair<create_uvec2_K, Range3>> vu; std::vector<std::pair<coeffs2_K, Range3>> vc;
  for (int b = 0; b < un->nfabs(); b++) {
    const vdn_box &bx = un->vbox[b];
    BoxP bp = make_boxp(un, b, bct);
    Uv2Args A;
    for (int d = 0; d < 2; d++) { A.lo[d] = bx.lo[d]; A.hi[d] = bx.hi[d]; A.phys[d][0] = bp.phys[d][0]; A.phys[d][1] = bp.phys[d][1]; }
    A.proj_type = proj_type; A.dt = dt; A.dtinv = 1.0 / dt;
    vu.push_back({ create_uvec2_K{ un->fabs[b], uo->fabs[b], rhh->fabs[b], gpp->fabs[b], A }, rng2(bx.lo[0] - un->ng, bx.hi[0] + un->ng, bx.lo[1] - un->ng, bx.hi[1] + un->ng) });
    vc.push_back({ coeffs2_K{ coeffs->fabs[b], rhh->fabs[b] }, rng2(bx.lo[0], bx.hi[0], bx.lo[1], bx.hi[1]) });
  }
  run_cells(vu); run_cells(vc);
  mf_fill_boundary(un); mf_fill_boundary(coeffs);
  double rel = ctx().prm.hg_rel_eps > 0.0 ? ctx().prm.hg_rel_eps : 1.e-12;
  double abs_eps = -1.0;
  if (proj_type == VDN_INITIAL_PROJECTION && ctx().prm.prob_type == 4) abs_eps = 1.e-12;
  int ebc[3][2];
  for (int d = 0; d < 3; d++) for (int s = 0; s < 2; s++) ebc[d][s] = d < 2 ? bct->ell_bc(0, 0, d, s, press_comp0) : VDN_BC_INT;
  NdRequest q;
  q.rh = rh; q.phi = phi; q.coeffs = coeffs; q.u = un; q.dx = dx; q.bc = ebc; q.rel_eps = rel; q.abs_eps = abs_eps; q.max_iter = ctx().prm.hg_max_iter;
  const int rc = nd2_solve(q);
  ctx().solver_cycles[1] = q.cycles; ctx().solver_res0[1] = q.res0; ctx().solver_res[1] = q.res;
  solver_check(rc, "nodal multigrid (2-D)", q.cycles, q.res, q.res0);
  if (proj_type == VDN_INITIAL_PROJECTION || proj_type == VDN_DIVU_ITERS) { mf_setval(gpp, 0.0, 0, gpp->nc, true); mf_setval(pp, 0.0, 0, 1, true); }
  std::vector<std::pair<hg_update2_K, Range3>> vh;
  for (int b = 0; b < un->nfabs(); b++) {
    const vdn_box &bx = un->vbox[b];
    Hg2Args H; H.hi[0] = bx.hi[0]; H.hi[1] = bx.hi[1]; H.dt = dt; H.dtinv = 1.0 / dt; H.dxi[0] = 1.0 / dx[0]; H.dxi[1] = 1.0 / dx[1]; H.proj_type = proj_type;
    vh.push_back({ hg_update2_K{ un->fabs[b], uo->fabs[b], gpp->fabs[b], rhh->fabs[b], pp->fabs[b], phi->fabs[b], H }, rng2(bx.lo[0], bx.hi[0] + 1, bx.lo[1], bx.hi[1] + 1) });
  }
  run_cells(vh);
  mf_fill_boundary(gpp); mf_fill_boundary(pp);
  mf_temp_free(coeffs); mf_temp_free(phi); mf_temp_free(rh);
  arena_release(mark);
}
