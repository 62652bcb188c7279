// krylov_wg.h -- Krylov bottom solvers run by ONE workgroup (vdn_params.mg_bottom_solver / hg_bottom_solver).
//
// wg_krylov<METHOD>(lv, K) solves  A x = b  on the coarsest level of a multigrid from the guess x = 0 (what a V-cycle's error equation starts from):
// METHOD 2 = conjugate gradients, METHOD 1 = BiCGStab, both preconditioned by the diagonal the level's operator returns.  It is a workgroup device
// function in the style of wg_cc_gsrb / wg_nd_jacobi: called by a one-workgroup kernel of its own (kk_bottom_krylov<LV>, below) and from inside the
// tail-cycle kernels (wg_krylov_any).  `lv` adapts a level: ONE struct per multigrid that holds the level by value, so the same object is a kernel
// argument, the adapter on the device and what the host sizes its launches from (CcKrylov in mg_cc.hip, NdKrylov in mg_nd.hip, C2Krylov and N2Krylov
// in dim2.hip):
//   count()                        points the workgroup strides over
//   point(t, c, i, j, k)           point t: its array offset and indices; false = not a candidate unknown (nodal Dirichlet nodes, periodic images)
//   apply(v, c, i, j, k, Av, diag) the level's operator on the array v (cc_apply / nd_apply as they are)
//   fill(v)                        periodic images of v (wg_cc_periodic / wg_nd_fill as they are; ends in a barrier when it does anything)
//   fill_count(), fill_point(v, t) the same fill one entry at a time, for the grid-wide form (krylov_grid.h)
//   size(), rhs(), x(), singular()
// count(), fill_count(), size() and singular() are pure integer work and KRY_HD: the host (mg_krylov_visit) asks the adapter for them.
//
// Unknowns: candidate points whose diagonal is not zero.  Everything else keeps x = 0, has zero residual and search direction and takes part in no
// dot product (a periodic nodal direction stores node n as an image of node 0: counted once, written by fill()).
// Dot products and norms: per-thread partial sums over the thread's points in ascending order, a butterfly over the 64 lanes of a wave, one LDS slot
// per wave, then EVERY thread adds the slots in ascending order.  No atomics: the same bits on every run and on every rank that holds the level, and
// every thread holds the same value -- each exit below is decided from such a value, so the whole workgroup leaves a loop together and no barrier
// sits in a divergent branch.
// Singular systems (no Dirichlet face, no alpha term): the mean of b over the unknowns is taken off before the iteration, the mean of x after it.
// Stopping: max |r| <= eps * max |b| (b after the mean went).  b = 0 (or not finite) returns x = 0 at once.
// Cap: 12 N iterations, N the level's largest extent (KrylovArgs::maxit, set by the host): diagonally preconditioned CG on the 25^3 bottom of a 200^3
// problem takes 233 to reduce the residual by 1e-10, 93 to the default 1e-3.  Every loop is bounded by it; no grid-wide barrier, no spin-wait.
// Breakdown (rho or omega zero or not finite, p.Ap <= 0, a residual that is not finite): the iteration stops BEFORE the update that would use the
// value, x keeps the last iterate, the event is counted and the V-cycle goes on.  x is only ever updated with finite coefficients.
// Work arrays, each of the level's padded size: CG 4 (r, p, q, 1/diag), BiCGStab 7 (r -- which also holds s --, r0, p, v, t, the preconditioned
// vector, 1/diag).  The workgroup zeroes them on entry (ghost entries outside a physical face must read as zero).
#pragma once
#include <type_traits>
#include "vdn_dev.h"      // (METHOD: VDN_KRYLOV_BICGSTAB, VDN_KRYLOV_CG of mg_plan.h)

#define KRY_HD __host__ __device__ __forceinline__      // the pure-integer members of a level adapter and the count helpers they call

struct KrylovArgs {
  double *w;          // 4 (CG) or 7 (BiCGStab) arrays of the bottom level's padded size, from the arena
  double *stats;      // 4 counters kept as doubles: bottom calls, total iterations, maximum iterations, breakdowns
  double eps;
  int maxit;
};

// sums s[0..NS) and maxima m[0..NM) over the workgroup; on return every thread holds the same totals.  blockDim.x is a multiple of 64, at most 1024.
template <int NS, int NM> DEVI void wg_reduce(double *s, double *m) {
  __shared__ double sm_[16 * (NS + NM)];
  #pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    #pragma unroll
    for (int q = 0; q < NS; q++) s[q] = s[q] + __shfl_xor(s[q], off, 64);
    #pragma unroll
    for (int q = 0; q < NM; q++) m[q] = nmax(m[q], __shfl_xor(m[q], off, 64));
  }
  const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    #pragma unroll
    for (int q = 0; q < NS; q++) sm_[wave * (NS + NM) + q] = s[q];
    #pragma unroll
    for (int q = 0; q < NM; q++) sm_[wave * (NS + NM) + NS + q] = m[q];
  }
  __syncthreads();
  #pragma unroll
  for (int q = 0; q < NS; q++) { double a = sm_[q]; for (int w = 1; w < nw; w++) a = a + sm_[w * (NS + NM) + q]; s[q] = a; }
  #pragma unroll
  for (int q = 0; q < NM; q++) { double a = sm_[NS + q]; for (int w = 1; w < nw; w++) a = nmax(a, sm_[w * (NS + NM) + NS + q]); m[q] = a; }
  __syncthreads();      // the slots are free again
}
DEVI bool kry_finite(double v) { return fabs(v) < __builtin_huge_val(); }      // false for NaN too

template <int METHOD, class LV> DEVI void wg_krylov(const LV &lv, const KrylovArgs &K) {
  constexpr int NW = (METHOD == VDN_KRYLOV_CG) ? 4 : 7;
  const long sz = lv.size();
  const int np = lv.count();
  double *x = lv.x();
  const double *b = lv.rhs();
  double *r = K.w, *p = K.w + sz, *q = K.w + 2 * sz, *dinv = K.w + (NW - 1) * sz;
  for (long t = threadIdx.x; t < (long)NW * sz; t += blockDim.x) K.w[t] = 0.0;
  __syncthreads();
  // 1 / diag on the unknowns, the sum of b over them and their number
  double s2[2] = { 0.0, 0.0 }, m1[1] = { 0.0 };
  for (int t = threadIdx.x; t < np; t += blockDim.x) {
    long c; int i, j, k;
    const bool cand = lv.point(t, c, i, j, k);
    x[c] = 0.0;
    if (cand) {
      double Av, diag; lv.apply(b, c, i, j, k, Av, diag);        // (only diag is used: it does not depend on the array)
      if (diag != 0.0) { dinv[c] = 1.0 / diag; s2[0] = s2[0] + b[c]; s2[1] = s2[1] + 1.0; }
    }
  }
  wg_reduce<2, 0>(s2, m1);
  const double nunk = s2[1];
  const double bmean = (lv.singular() && nunk > 0.0) ? s2[0] / nunk : 0.0;
  // r = b - mean on the unknowns; CG: p = z = r / diag, rho = r.z
  double rho = 0.0, bn = 0.0;
  s2[0] = 0.0;
  for (int t = threadIdx.x; t < np; t += blockDim.x) {
    long c; int i, j, k;
    lv.point(t, c, i, j, k);
    const double di = dinv[c];
    if (di != 0.0) {
      const double rv = b[c] - bmean;
      r[c] = rv;
      if (METHOD == VDN_KRYLOV_CG) { const double z = rv * di; p[c] = z; s2[0] = s2[0] + rv * z; }
      else { q[c] = rv; s2[0] = s2[0] + rv * rv; }                 // q = r0 (BiCGStab's shadow residual); rho = r0.r
      m1[0] = nmax(m1[0], fabs(rv));
    }
  }
  wg_reduce<1, 1>(s2, m1);
  rho = s2[0]; bn = m1[0];
  int it = 0, broke = 0;
  const bool go = bn > 0.0 && kry_finite(bn) && kry_finite(rho);
  if (!go && !(bn == 0.0)) broke = 1;                              // a right-hand side that is not finite: x = 0, counted
  const double tol = K.eps * bn;
  if (go) {
    if (METHOD == VDN_KRYLOV_CG) {
      while (it < K.maxit) {
        __syncthreads();                                           // p complete
        lv.fill(p);
        double pq[1] = { 0.0 };
        for (int t = threadIdx.x; t < np; t += blockDim.x) {
          long c; int i, j, k;
          lv.point(t, c, i, j, k);
          if (dinv[c] != 0.0) { double Av, diag; lv.apply(p, c, i, j, k, Av, diag); q[c] = Av; pq[0] = pq[0] + p[c] * Av; }
        }
        wg_reduce<1, 0>(pq, m1);
        if (!(pq[0] > 0.0) || !kry_finite(pq[0])) { broke = 1; break; }
        const double alpha = rho / pq[0];
        if (!kry_finite(alpha)) { broke = 1; break; }
        double rz[1] = { 0.0 }, rn[1] = { 0.0 };
        for (int t = threadIdx.x; t < np; t += blockDim.x) {
          long c; int i, j, k;
          lv.point(t, c, i, j, k);
          const double di = dinv[c];
          if (di != 0.0) {
            x[c] = x[c] + alpha * p[c];
            const double rv = r[c] - alpha * q[c];
            r[c] = rv;
            rz[0] = rz[0] + rv * (rv * di);
            rn[0] = nmax(rn[0], fabs(rv));
          }
        }
        wg_reduce<1, 1>(rz, rn);
        it++;
        if (!kry_finite(rn[0])) { broke = 1; break; }
        if (rn[0] <= tol) break;
        if (!(rz[0] > 0.0) || !kry_finite(rz[0])) { broke = 1; break; }
        const double beta = rz[0] / rho;
        rho = rz[0];
        for (int t = threadIdx.x; t < np; t += blockDim.x) {
          long c; int i, j, k;
          lv.point(t, c, i, j, k);
          const double di = dinv[c];
          if (di != 0.0) p[c] = r[c] * di + beta * p[c];
        }
      }
    } else {
      double *r0 = q, *v = K.w + 3 * sz, *tt = K.w + 4 * sz, *ph = K.w + 5 * sz;
      double alpha = 1.0, omega = 1.0, rho_old = 1.0;
      while (it < K.maxit) {
        if (rho == 0.0 || !kry_finite(rho)) { broke = 1; break; }
        const double beta = (rho / rho_old) * (alpha / omega);
        if (!kry_finite(beta)) { broke = 1; break; }
        for (int t = threadIdx.x; t < np; t += blockDim.x) {      // p = r + beta (p - omega v); ph = p / diag  (first pass: p = v = 0)
          long c; int i, j, k;
          lv.point(t, c, i, j, k);
          const double di = dinv[c];
          if (di != 0.0) { const double pv = r[c] + beta * (p[c] - omega * v[c]); p[c] = pv; ph[c] = pv * di; }
        }
        __syncthreads();
        lv.fill(ph);
        double s1[1] = { 0.0 };
        for (int t = threadIdx.x; t < np; t += blockDim.x) {
          long c; int i, j, k;
          lv.point(t, c, i, j, k);
          if (dinv[c] != 0.0) { double Av, diag; lv.apply(ph, c, i, j, k, Av, diag); v[c] = Av; s1[0] = s1[0] + r0[c] * Av; }
        }
        wg_reduce<1, 0>(s1, m1);
        if (s1[0] == 0.0 || !kry_finite(s1[0])) { broke = 1; break; }
        alpha = rho / s1[0];
        if (!kry_finite(alpha)) { broke = 1; break; }
        double sn[1] = { 0.0 };
        for (int t = threadIdx.x; t < np; t += blockDim.x) {      // x += alpha ph; s = r - alpha v (kept in r); ph = s / diag
          long c; int i, j, k;
          lv.point(t, c, i, j, k);
          const double di = dinv[c];
          if (di != 0.0) {
            x[c] = x[c] + alpha * ph[c];
            const double sv = r[c] - alpha * v[c];
            r[c] = sv; ph[c] = sv * di;
            sn[0] = nmax(sn[0], fabs(sv));
          }
        }
        wg_reduce<0, 1>(s1, sn);                                   // (its barriers also complete ph)
        it++;
        if (!kry_finite(sn[0])) { broke = 1; break; }
        if (sn[0] <= tol) break;
        lv.fill(ph);
        double ts[2] = { 0.0, 0.0 };
        for (int t = threadIdx.x; t < np; t += blockDim.x) {
          long c; int i, j, k;
          lv.point(t, c, i, j, k);
          if (dinv[c] != 0.0) { double Av, diag; lv.apply(ph, c, i, j, k, Av, diag); tt[c] = Av; ts[0] = ts[0] + Av * r[c]; ts[1] = ts[1] + Av * Av; }
        }
        wg_reduce<2, 0>(ts, m1);
        if (!(ts[1] > 0.0) || !kry_finite(ts[1]) || !kry_finite(ts[0])) { broke = 1; break; }
        omega = ts[0] / ts[1];
        if (omega == 0.0 || !kry_finite(omega)) { broke = 1; break; }
        double rr[1] = { 0.0 }, rn[1] = { 0.0 };
        for (int t = threadIdx.x; t < np; t += blockDim.x) {      // x += omega ph; r = s - omega t; rho = r0.r
          long c; int i, j, k;
          lv.point(t, c, i, j, k);
          if (dinv[c] != 0.0) {
            x[c] = x[c] + omega * ph[c];
            const double rv = r[c] - omega * tt[c];
            r[c] = rv;
            rr[0] = rr[0] + r0[c] * rv;
            rn[0] = nmax(rn[0], fabs(rv));
          }
        }
        wg_reduce<1, 1>(rr, rn);
        if (!kry_finite(rn[0])) { broke = 1; break; }
        if (rn[0] <= tol) break;
        rho_old = rho; rho = rr[0];
      }
    }
  }
  __syncthreads();
  if (lv.singular() && nunk > 0.0) {                               // the mean of x over the same set
    double sx[1] = { 0.0 };
    for (int t = threadIdx.x; t < np; t += blockDim.x) {
      long c; int i, j, k;
      lv.point(t, c, i, j, k);
      if (dinv[c] != 0.0) sx[0] = sx[0] + x[c];
    }
    wg_reduce<1, 0>(sx, m1);
    const double xm = sx[0] / nunk;
    if (kry_finite(xm))
      for (int t = threadIdx.x; t < np; t += blockDim.x) {
        long c; int i, j, k;
        lv.point(t, c, i, j, k);
        if (dinv[c] != 0.0) x[c] = x[c] - xm;
      }
    __syncthreads();
  }
  lv.fill(x);
  if (threadIdx.x == 0) {
    K.stats[0] = K.stats[0] + 1.0;
    K.stats[1] = K.stats[1] + (double)it;
    if ((double)it > K.stats[2]) K.stats[2] = (double)it;
    K.stats[3] = K.stats[3] + (double)broke;
  }
  __syncthreads();
}
template <class LV> DEVI void wg_krylov_any(int method, const LV &lv, const KrylovArgs &K) {      // method: uniform over the launch
  if (method == VDN_KRYLOV_CG) wg_krylov<VDN_KRYLOV_CG>(lv, K); else wg_krylov<VDN_KRYLOV_BICGSTAB>(lv, K);
}
// the one-workgroup bottom visit of every multigrid (mg_krylov_visit in krylov_grid.h launches it: dim3(1), 1024 threads)
template <class LV> __global__ void __launch_bounds__(1024) kk_bottom_krylov(LV lv, KrylovArgs K, int method) { wg_krylov_any(method, lv, K); }
// What a tail-cycle kernel takes besides its levels: nothing in the sweeps instantiation, the solve's arguments in the Krylov one
// (singular: the cell-centred hierarchy's flag; a nodal level knows its own)
struct KrylovTailArgs { KrylovArgs K; int method, singular; };
struct NoKrylovTailArgs {};
template <bool KRYLOV> using KrylovTail = std::conditional_t<KRYLOV, KrylovTailArgs, NoKrylovTailArgs>;
