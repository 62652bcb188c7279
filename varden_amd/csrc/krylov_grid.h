// krylov_grid.h -- the Krylov bottom solvers of krylov_wg.h run by the WHOLE GPU, for bottom levels too large for one workgroup.
//
// The same preconditioned CG / BiCGStab as wg_krylov -- the same unknowns (candidate points with a non-zero diagonal), the diagonal of the level's operator as
// preconditioner, x = 0 to start from, the mean of b taken off before and the mean of x after the iteration on singular systems, max |r| <= eps max |b| to
// stop, b = 0 returns x = 0, the cap of 12 N iterations, a breakdown stops BEFORE the update that would use the bad value and is counted -- as a short, fixed
// sequence of plain launches on the solve's stream.  No cooperative launch, no grid-wide barrier, no spin-wait, no atomics; every loop in a kernel is bounded.
// `LV` is the level adapter wg_krylov takes, handed to a kernel by value (CcKrylov in mg_cc.hip, NdKrylov in mg_nd.hip, C2Krylov and N2Krylov in dim2.hip); used here besides what
// wg_krylov uses: fill_count() and fill_point(v, t), the periodic fill of the level one point at a time (what wg_cc_periodic / wg_nd_fill loop over).
// mg_krylov_visit (at the end) is the one bottom visit of all four multigrids: one workgroup (kk_bottom_krylov) or this form, sized from the adapter itself.
//
// Launch shape (krylov_grid_shape): a function of the number of points alone -- 256, 512 or 1024 threads per workgroup, at most KG_MAXWG workgroups, grid-stride
// over the points.  Never a CU count: the replicated tail gives the same bits on every rank and on every run.
// Sums: per-thread partial sums over the thread's points in ascending order, wg_reduce within the workgroup (its fixed order), ONE partial per workgroup and
// quantity stored in K.part; whoever consumes the sum adds the partials in ascending workgroup order (kg_sum, every thread the same loop: every thread of every
// workgroup holds the same bits, so every exit below is taken by the whole grid).
// Scalars: the step that turns sums into alpha, beta, omega and the stopping decisions is the prologue of the next kernel.  It lives in two state blocks of
// KG_NST doubles, K.st: the kernels of iteration k read block k & 1 (complete since the last kernel of iteration k - 1) and thread 0 of workgroup 0 builds block
// (k + 1) & 1 up -- a field written by one kernel of the iteration is read only by LATER kernels of it, never by the kernel that writes it.  H0..H3 say that
// kernel 0..3 of the iteration stopped it (1 converged or capped, 2 breakdown); the last kernel of the iteration folds them into DONE, and a kernel that finds
// DONE set returns at once: the launches of a visit after convergence are no-ops.
// The host launches `budget` iterations per visit without reading anything back (the V-cycles are captured into hipGraphs): the cap itself on the first solve of
// a kind, then what the previous solve of that kind needed plus a margin (bottom_budget_begin in runtime.hip), never more than the cap.  A visit that runs out of
// budget leaves the iterate it has -- finite, mean removed, periodic images filled -- and is counted (stats[8 + which]); the next solve then carries twice the budget.
//
// CG, per iteration:        [fill p]  kg_cg_apply (q = A p, p.q)   kg_cg_update (alpha; x, r; r.z, max |r|)   kg_cg_dir (stop?; beta; p)
// BiCGStab, per iteration:  kg_bi_dir (stop?; rho, beta; p, ph)  [fill ph]  kg_bi_apply1 (v = A ph, r0.v)  kg_bi_half (alpha; x, s, ph; max |s|)  [fill ph]
//                           kg_bi_apply2 (stop?; t = A ph, t.s, t.t)  kg_bi_full (omega; x, r; r0.r, max |r|)
// Per visit: memset of the work arrays, kg_init0 (x = 0, 1 / diag, sum and number of b), kg_init1 (r, p or r0; rho, max |b|), kg_start (one workgroup: the state
// blocks), the iterations, [kg_xsum] kg_finish (mean of x, the statistics) [fill x].  The work arrays are those of wg_krylov (4 / 7 of the level's padded size).
#pragma once
#include "krylov_wg.h"

// Smallest bottom level (points: cells, or nodes) that takes this form: the smallest measured size from which it is not slower than one workgroup.
// tools/bottom_solver_probe.py 34,50,66,90 5 3 cg <library>, the library built with this constant at 2^30 and at 0 (MI355X, CG / CG, five steps after two
// warm-up steps; MAC + HG phase per step in ms, each phase 7-8 / 10 bottom visits; profiles/bottom_solver_probe_wide.txt):
//   bottom (cells, nodes)   CG iterations per visit   one workgroup     grid-wide
//   17^3, 18^3              29, 18                     6.23 +  6.22      6.10 +  6.12
//   25^3, 26^3              41, 22                    17.69 + 18.25      9.35 +  8.54
//   33^3, 34^3              52, 27                    52.51 + 48.31     19.08 + 15.85
//   45^3, 46^3              69, 34                   181.57 + 161.61    32.41 + 22.01
// Not below 22 x 11 x 11 cells / 23 x 12 x 12 nodes: the largest bottom level of tests/test_bottom_solver_gpu.py, which stays one workgroup.
#ifndef VDN_KRYLOV_GRID_MIN_POINTS
#define VDN_KRYLOV_GRID_MIN_POINTS 4913
#endif
// The same for the two dm = 2 multigrids (dim2.hip), whose crossover lies higher: their V-cycles are plain launches, not hipGraphs, so an iteration of this form
// costs its three to seven launches on the host as well (the launches a visit's budget leaves over after convergence included), and the 5- and 9-point operators
// leave a workgroup less to do per point than the 7- and 27-point ones.  tools/bottom_solver_probe.py 102,142,154,162,170,182,202,282 5 2 cg <library>, the
// library built with this constant at 2^30 and at 0 (MI355X, CG / CG, five steps after two warm-up steps; MAC + HG phase per step in ms, each phase 6 / 10 bottom
// visits; every figure repeated within 0.1 ms (one workgroup) and 1.3 ms (grid-wide) by a second run; profiles/bottom_solver_probe_2d_wide.txt):
//   bottom (cells, nodes)   CG iterations per visit   one workgroup     grid-wide
//   51^2, 52^2               88, 38                     5.86 +  5.24     11.57 + 10.96
//   71^2, 72^2              115, 49                    11.49 +  9.91     15.80 + 14.87
//   77^2, 78^2              123, 52                    13.95 + 12.16     16.55 + 18.62
//   81^2, 82^2              128, 55                    15.41 + 13.61     17.06 + 18.33
//   85^2, 86^2              134, 58                    17.42 + 15.26     17.74 + 18.39
//   91^2, 92^2              146, 62                    21.18 + 18.18     20.10 + 19.00
//   101^2, 102^2            164, 68                    28.12 + 23.80     22.78 + 21.23
//   141^2, 142^2            218, 93                    67.40 + 57.56     38.52 + 34.05
// 101^2 is the smallest measured size from which neither operator is slower (at 91^2 the nodal one still is).  Not below 23 x 12 nodes: the largest bottom
// level of tests/test_bottom_solver_2d_gpu.py, which stays one workgroup.
#ifndef VDN_KRYLOV_GRID_MIN_POINTS_2D
#define VDN_KRYLOV_GRID_MIN_POINTS_2D 10201
#endif

#define KG_MAXWG 256
enum { KG_SB = 0, KG_CNT, KG_RHO, KG_BN, KG_D0, KG_D1, KG_E0, KG_E1, KG_SN, KG_X, KG_NPART };
enum { KG_DONE = 0, KG_IT, KG_BROKE, KG_SRHO, KG_RHO_OLD, KG_ALPHA, KG_OMEGA, KG_TOL, KG_NUNK, KG_BMEAN, KG_PEND, KG_H0, KG_H1, KG_H2, KG_H3, KG_NST = 16 };
#define KG_DOUBLES (KG_NPART * KG_MAXWG + 2 * KG_NST)      // partials and state blocks behind the work arrays

struct KrylovGridArgs {
  double *w;          // KrylovArgs::w
  double *part;       // KG_NPART areas of KG_MAXWG partial sums, then the two state blocks
  double *stats;      // KrylovArgs::stats
  double *exhausted;  // visits that ran out of budget before they stopped
  double eps;
  int maxit;
  DEVI double *st(int b) const { return part + KG_NPART * KG_MAXWG + b * KG_NST; }
};

// What a hierarchy (CCMG, NDMG; dm = 2: CC2MG, ND2MG) keeps of its Krylov bottom solver.  w: the work arrays, of the bottom level's padded size (nullptr = the bottom sweeps);
// part: the grid-wide form's partial sums and state blocks, on a bottom level of VDN_KRYLOV_GRID_MIN_POINTS (dm = 2: ..._2D) points (cells, or nodes) or more; budget: the
// iterations a visit of that form launches; kind: its key in bottom_budget_begin.
struct MgKrylov { double *w = nullptr; int method = 0, maxit = 0; double *part = nullptr; int budget = 0; unsigned long long kind = 0; };
// The set-up both builds share.  The arrays come from the arena here, so their addresses repeat with the hierarchy's.  sz: the bottom level's padded size;
// N: its largest extent in points; np: its points; kind: what tells one solver's bottom systems apart (solver, method, extents, boundary, tolerance);
// min_points: the crossover of the caller's multigrids
inline void mg_krylov_setup(MgKrylov &K, int method, long sz, int N, long np, const GraphKey &kind, long min_points = VDN_KRYLOV_GRID_MIN_POINTS) {
  K.method = method;
  K.w = (double *)arena_alloc(sizeof(double) * sz * (method == VDN_KRYLOV_CG ? 4 : 7));
  K.maxit = 12 * N;
  if (np >= min_points) {
    K.part = (double *)arena_alloc(sizeof(double) * KG_DOUBLES);
    K.kind = kind.h | 1ull;
    K.budget = K.maxit;
  }
}
// The start of one solve of multigrid `which` (0 cell-centred, 1 nodal): the form vdn_last_bottom_form reports; then, when `selected`, the iteration budget of this kind of bottom
// system (bottom_budget_begin reads the previous solve's statistics: before they are reset) and the statistics, which are those of one solve.
// The callers differ in when they call and in `selected`, and so in what vdn_last_bottom_stats reports for a bottom that keeps its sweeps although a method is selected:
//   3-D (cc_solve, nd_solve): not on a kept, already-built hierarchy running fixed cycles (a composite solve's statistics are those of all its cycles); selected = kry.w is
//       set, so such a bottom leaves the statistics of the last Krylov solve standing;
//   2-D (cc2_solve, nd2_solve): every solve; selected = a method is selected, one-level hierarchies that keep their sweeps included, so such a bottom reports zeros.
inline void mg_krylov_begin(MgKrylov &K, int which, bool selected) {
  bottom_form_set(which, K.w ? (K.part ? 2 : 1) : 0);
  if (!selected) return;
  const int budget = bottom_budget_begin(which, K.kind, K.maxit);
  if (K.part) K.budget = budget;
  bottom_stats_reset(which);
}

DEVI double kg_sum(const double *p, int n) { double a = p[0]; for (int g = 1; g < n; g++) a = a + p[g]; return a; }
DEVI double kg_max(const double *p, int n) { double a = p[0]; for (int g = 1; g < n; g++) a = nmax(a, p[g]); return a; }
DEVI bool kg_first() { return blockIdx.x == 0 && threadIdx.x == 0; }
DEVI void kg_put(const KrylovGridArgs &K, int area, double v) { if (threadIdx.x == 0) K.part[area * KG_MAXWG + blockIdx.x] = v; }
DEVI const double *kg_part(const KrylovGridArgs &K, int area) { return K.part + area * KG_MAXWG; }
// the fields every iteration hands on unchanged
DEVI void kg_carry(double *N, const double *S) {
  N[KG_SRHO] = S[KG_SRHO]; N[KG_RHO_OLD] = S[KG_RHO_OLD]; N[KG_ALPHA] = S[KG_ALPHA]; N[KG_OMEGA] = S[KG_OMEGA];
  N[KG_TOL] = S[KG_TOL]; N[KG_NUNK] = S[KG_NUNK]; N[KG_BMEAN] = S[KG_BMEAN]; N[KG_PEND] = S[KG_PEND];
}
#define KG_POINTS(t, np) for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < (np); t += gridDim.x * blockDim.x)

// ---- start of a visit ---------------------------------------------------------------------------------------------------------------------
template <int METHOD, class LV> __global__ void __launch_bounds__(1024) kg_init0(LV lv, KrylovGridArgs K) {
  constexpr int NW = (METHOD == VDN_KRYLOV_CG) ? 4 : 7;
  const int np = lv.count();
  double *x = lv.x();
  const double *b = lv.rhs();
  double *dinv = K.w + (NW - 1) * lv.size();
  double s2[2] = { 0.0, 0.0 }, m1[1] = { 0.0 };
  KG_POINTS(t, np) {
    long c; int i, j, k;
    const bool cand = lv.point(t, c, i, j, k);
    x[c] = 0.0;
    if (cand) {
      double Av, diag; lv.apply(b, c, i, j, k, Av, diag);
      if (diag != 0.0) { dinv[c] = 1.0 / diag; s2[0] = s2[0] + b[c]; s2[1] = s2[1] + 1.0; }
    }
  }
  wg_reduce<2, 0>(s2, m1);
  kg_put(K, KG_SB, s2[0]); kg_put(K, KG_CNT, s2[1]);
}
template <int METHOD, class LV> __global__ void __launch_bounds__(1024) kg_init1(LV lv, KrylovGridArgs K) {
  constexpr int NW = (METHOD == VDN_KRYLOV_CG) ? 4 : 7;
  const long sz = lv.size();
  const int np = lv.count();
  const double *b = lv.rhs();
  double *r = K.w, *p = K.w + sz, *q = K.w + 2 * sz, *dinv = K.w + (NW - 1) * sz;
  const double nunk = kg_sum(kg_part(K, KG_CNT), gridDim.x);
  const double bmean = (lv.singular() && nunk > 0.0) ? kg_sum(kg_part(K, KG_SB), gridDim.x) / nunk : 0.0;
  double s1[1] = { 0.0 }, m1[1] = { 0.0 };
  KG_POINTS(t, np) {
    long c; int i, j, k;
    lv.point(t, c, i, j, k);
    const double di = dinv[c];
    if (di != 0.0) {
      const double rv = b[c] - bmean;
      r[c] = rv;
      if (METHOD == VDN_KRYLOV_CG) { const double z = rv * di; p[c] = z; s1[0] = s1[0] + rv * z; }
      else { q[c] = rv; s1[0] = s1[0] + rv * rv; }
      m1[0] = nmax(m1[0], fabs(rv));
    }
  }
  wg_reduce<1, 1>(s1, m1);
  kg_put(K, KG_RHO, s1[0]); kg_put(K, KG_BN, m1[0]);
}
// one workgroup: both state blocks
static __global__ void __launch_bounds__(64) kg_start(KrylovGridArgs K, int nwg, int singular) {
  const double nunk = kg_sum(kg_part(K, KG_CNT), nwg);
  const double bmean = (singular && nunk > 0.0) ? kg_sum(kg_part(K, KG_SB), nwg) / nunk : 0.0;
  const double rho = kg_sum(kg_part(K, KG_RHO), nwg), bn = kg_max(kg_part(K, KG_BN), nwg);
  const bool go = bn > 0.0 && kry_finite(bn) && kry_finite(rho);
  if (threadIdx.x < 2 * KG_NST) K.st(0)[threadIdx.x] = 0.0;
  __syncthreads();
  if (threadIdx.x == 0) {
    double *S = K.st(0);
    S[KG_DONE] = go ? 0.0 : 1.0;
    S[KG_BROKE] = (!go && !(bn == 0.0)) ? 1.0 : 0.0;                 // a right-hand side that is not finite: x = 0, counted
    S[KG_SRHO] = rho; S[KG_RHO_OLD] = 1.0; S[KG_ALPHA] = 1.0; S[KG_OMEGA] = 1.0;
    S[KG_TOL] = K.eps * bn; S[KG_NUNK] = nunk; S[KG_BMEAN] = bmean;
  }
}
// periodic images of work array `a` (of x itself: a < 0); cur >= 0: not once the solve is done
template <class LV> __global__ void __launch_bounds__(256) kg_fill(LV lv, KrylovGridArgs K, int a, int cur) {
  if (cur >= 0 && K.st(cur)[KG_DONE] != 0.0) return;
  double *v = a < 0 ? lv.x() : K.w + (long)a * lv.size();
  const int nf = lv.fill_count();
  KG_POINTS(t, nf) lv.fill_point(v, t);
}

// ---- conjugate gradients ----------------------------------------------------------------------------------------------------------------------
template <class LV> __global__ void __launch_bounds__(1024) kg_cg_apply(LV lv, KrylovGridArgs K, int cur) {
  if (K.st(cur)[KG_DONE] != 0.0) return;
  const long sz = lv.size();
  const int np = lv.count();
  const double *p = K.w + sz, *dinv = K.w + 3 * sz;
  double *q = K.w + 2 * sz;
  double pq[1] = { 0.0 }, m1[1] = { 0.0 };
  KG_POINTS(t, np) {
    long c; int i, j, k;
    lv.point(t, c, i, j, k);
    if (dinv[c] != 0.0) { double Av, diag; lv.apply(p, c, i, j, k, Av, diag); q[c] = Av; pq[0] = pq[0] + p[c] * Av; }
  }
  wg_reduce<1, 0>(pq, m1);
  kg_put(K, KG_D0, pq[0]);
}
template <class LV> __global__ void __launch_bounds__(1024) kg_cg_update(LV lv, KrylovGridArgs K, int cur) {
  const double *S = K.st(cur);
  double *N = K.st(cur ^ 1);
  if (S[KG_DONE] != 0.0) return;
  const double pq = kg_sum(kg_part(K, KG_D0), gridDim.x);
  const double alpha = S[KG_SRHO] / pq;
  if (!(pq > 0.0) || !kry_finite(pq) || !kry_finite(alpha)) { if (kg_first()) N[KG_H1] = 2.0; return; }
  const long sz = lv.size();
  const int np = lv.count();
  double *x = lv.x(), *r = K.w;
  const double *p = K.w + sz, *q = K.w + 2 * sz, *dinv = K.w + 3 * sz;
  double rz[1] = { 0.0 }, rn[1] = { 0.0 };
  KG_POINTS(t, np) {
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
  kg_put(K, KG_E0, rz[0]); kg_put(K, KG_E1, rn[0]);
}
template <class LV> __global__ void __launch_bounds__(1024) kg_cg_dir(LV lv, KrylovGridArgs K, int cur) {
  const double *S = K.st(cur);
  double *N = K.st(cur ^ 1);
  if (S[KG_DONE] != 0.0) { if (kg_first()) { kg_carry(N, S); N[KG_DONE] = 1.0; N[KG_IT] = S[KG_IT]; N[KG_BROKE] = S[KG_BROKE]; } return; }
  if (N[KG_H1] != 0.0) { if (kg_first()) { kg_carry(N, S); N[KG_DONE] = 1.0; N[KG_IT] = S[KG_IT]; N[KG_BROKE] = S[KG_BROKE] + 1.0; } return; }
  const double rz = kg_sum(kg_part(K, KG_E0), gridDim.x), rn = kg_max(kg_part(K, KG_E1), gridDim.x);
  const double it = S[KG_IT] + 1.0, rho = S[KG_SRHO];
  int done = 0, broke = 0;
  if (!kry_finite(rn)) { done = 1; broke = 1; }
  else if (rn <= S[KG_TOL]) done = 1;
  else if (!(rz > 0.0) || !kry_finite(rz)) { done = 1; broke = 1; }
  if (!done) {
    const double beta = rz / rho;
    const long sz = lv.size();
    const int np = lv.count();
    const double *r = K.w, *dinv = K.w + 3 * sz;
    double *p = K.w + sz;
    KG_POINTS(t, np) {
      long c; int i, j, k;
      lv.point(t, c, i, j, k);
      const double di = dinv[c];
      if (di != 0.0) p[c] = r[c] * di + beta * p[c];
    }
    if (it >= (double)K.maxit) done = 1;
  }
  if (kg_first()) {
    kg_carry(N, S);
    if (!broke && !(rn <= S[KG_TOL])) N[KG_SRHO] = rz;
    N[KG_DONE] = (double)done; N[KG_IT] = it; N[KG_BROKE] = S[KG_BROKE] + (double)broke;
  }
}

// ---- BiCGStab ---------------------------------------------------------------------------------------------------------------------------------
// arrays, in wg_krylov's order: r (also s), p, r0, v, t, ph (the preconditioned vector), 1 / diag.  PEND: kg_bi_full left r0.r and max |r| as partials; kg_bi_dir takes them up.
template <class LV> __global__ void __launch_bounds__(1024) kg_bi_dir(LV lv, KrylovGridArgs K, int cur) {
  const double *S = K.st(cur);
  double *N = K.st(cur ^ 1);
  if (S[KG_DONE] != 0.0) return;
  double rho = S[KG_SRHO], rho_old = S[KG_RHO_OLD];
  int code = 0;
  if (S[KG_PEND] != 0.0) {
    const double rr = kg_sum(kg_part(K, KG_E0), gridDim.x), rn = kg_max(kg_part(K, KG_E1), gridDim.x);
    if (!kry_finite(rn)) code = 2;
    else if (rn <= S[KG_TOL] || S[KG_IT] >= (double)K.maxit) code = 1;
    rho_old = rho; rho = rr;
  }
  if (!code && (rho == 0.0 || !kry_finite(rho))) code = 2;
  const double omega = S[KG_OMEGA];
  const double beta = (rho / rho_old) * (S[KG_ALPHA] / omega);
  if (!code && !kry_finite(beta)) code = 2;
  if (code) { if (kg_first()) N[KG_H0] = (double)code; return; }
  if (kg_first()) { N[KG_SRHO] = rho; N[KG_RHO_OLD] = rho_old; }
  const long sz = lv.size();
  const int np = lv.count();
  const double *r = K.w, *v = K.w + 3 * sz, *dinv = K.w + 6 * sz;
  double *p = K.w + sz, *ph = K.w + 5 * sz;
  KG_POINTS(t, np) {
    long c; int i, j, k;
    lv.point(t, c, i, j, k);
    const double di = dinv[c];
    if (di != 0.0) { const double pv = r[c] + beta * (p[c] - omega * v[c]); p[c] = pv; ph[c] = pv * di; }
  }
}
// SECOND = 0: v = A ph, r0.v.  SECOND = 1: the half step's stopping test, then t = A ph, t.s and t.t
template <int SECOND, class LV> __global__ void __launch_bounds__(1024) kg_bi_apply(LV lv, KrylovGridArgs K, int cur) {
  const double *S = K.st(cur);
  double *N = K.st(cur ^ 1);
  if (S[KG_DONE] != 0.0 || N[KG_H0] != 0.0) return;
  if (SECOND) {
    if (N[KG_H2] != 0.0) return;
    const double sn = kg_max(kg_part(K, KG_SN), gridDim.x);
    if (!kry_finite(sn)) { if (kg_first()) N[KG_H3] = 2.0; return; }
    if (sn <= S[KG_TOL]) { if (kg_first()) N[KG_H3] = 1.0; return; }
  }
  const long sz = lv.size();
  const int np = lv.count();
  const double *r = K.w, *r0 = K.w + 2 * sz, *ph = K.w + 5 * sz, *dinv = K.w + 6 * sz;
  double *out = K.w + (SECOND ? 4 : 3) * sz;
  double s2[2] = { 0.0, 0.0 }, m1[1] = { 0.0 };
  KG_POINTS(t, np) {
    long c; int i, j, k;
    lv.point(t, c, i, j, k);
    if (dinv[c] != 0.0) {
      double Av, diag; lv.apply(ph, c, i, j, k, Av, diag);
      out[c] = Av;
      if (SECOND) { s2[0] = s2[0] + Av * r[c]; s2[1] = s2[1] + Av * Av; } else s2[0] = s2[0] + r0[c] * Av;
    }
  }
  wg_reduce<2, 0>(s2, m1);
  kg_put(K, KG_D0, s2[0]); kg_put(K, KG_D1, s2[1]);
}
template <class LV> __global__ void __launch_bounds__(1024) kg_bi_half(LV lv, KrylovGridArgs K, int cur) {
  const double *S = K.st(cur);
  double *N = K.st(cur ^ 1);
  if (S[KG_DONE] != 0.0 || N[KG_H0] != 0.0) return;
  const double s1 = kg_sum(kg_part(K, KG_D0), gridDim.x);
  const double alpha = N[KG_SRHO] / s1;
  if (s1 == 0.0 || !kry_finite(s1) || !kry_finite(alpha)) { if (kg_first()) N[KG_H2] = 2.0; return; }
  if (kg_first()) N[KG_ALPHA] = alpha;
  const long sz = lv.size();
  const int np = lv.count();
  double *x = lv.x(), *r = K.w, *ph = K.w + 5 * sz;
  const double *v = K.w + 3 * sz, *dinv = K.w + 6 * sz;
  double s0[1] = { 0.0 }, sn[1] = { 0.0 };
  KG_POINTS(t, np) {
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
  wg_reduce<0, 1>(s0, sn);
  kg_put(K, KG_SN, sn[0]);
}
template <class LV> __global__ void __launch_bounds__(1024) kg_bi_full(LV lv, KrylovGridArgs K, int cur) {
  const double *S = K.st(cur);
  double *N = K.st(cur ^ 1);
  if (S[KG_DONE] != 0.0) { if (kg_first()) { kg_carry(N, S); N[KG_DONE] = 1.0; N[KG_IT] = S[KG_IT]; N[KG_BROKE] = S[KG_BROKE]; } return; }
  const double h0 = N[KG_H0], h2 = N[KG_H2], h3 = N[KG_H3];
  if (h0 != 0.0 || h2 != 0.0 || h3 != 0.0) {                      // (the half step counts as an iteration: it stopped after `it` went up)
    if (kg_first()) {
      N[KG_TOL] = S[KG_TOL]; N[KG_NUNK] = S[KG_NUNK]; N[KG_BMEAN] = S[KG_BMEAN]; N[KG_PEND] = 0.0; N[KG_OMEGA] = S[KG_OMEGA];
      N[KG_DONE] = 1.0; N[KG_IT] = S[KG_IT] + (h3 != 0.0 ? 1.0 : 0.0);
      N[KG_BROKE] = S[KG_BROKE] + ((h0 == 2.0 || h2 == 2.0 || h3 == 2.0) ? 1.0 : 0.0);
    }
    return;
  }
  const double ts0 = kg_sum(kg_part(K, KG_D0), gridDim.x), ts1 = kg_sum(kg_part(K, KG_D1), gridDim.x);
  const double omega = ts0 / ts1;
  if (!(ts1 > 0.0) || !kry_finite(ts1) || !kry_finite(ts0) || omega == 0.0 || !kry_finite(omega)) {
    if (kg_first()) {
      N[KG_TOL] = S[KG_TOL]; N[KG_NUNK] = S[KG_NUNK]; N[KG_BMEAN] = S[KG_BMEAN]; N[KG_PEND] = 0.0; N[KG_OMEGA] = S[KG_OMEGA];
      N[KG_DONE] = 1.0; N[KG_IT] = S[KG_IT] + 1.0; N[KG_BROKE] = S[KG_BROKE] + 1.0;
    }
    return;
  }
  const long sz = lv.size();
  const int np = lv.count();
  double *x = lv.x(), *r = K.w;
  const double *r0 = K.w + 2 * sz, *tt = K.w + 4 * sz, *ph = K.w + 5 * sz, *dinv = K.w + 6 * sz;
  double rr[1] = { 0.0 }, rn[1] = { 0.0 };
  KG_POINTS(t, np) {
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
  kg_put(K, KG_E0, rr[0]); kg_put(K, KG_E1, rn[0]);
  if (kg_first()) {
    N[KG_TOL] = S[KG_TOL]; N[KG_NUNK] = S[KG_NUNK]; N[KG_BMEAN] = S[KG_BMEAN]; N[KG_PEND] = 1.0; N[KG_OMEGA] = omega;
    N[KG_DONE] = 0.0; N[KG_IT] = S[KG_IT] + 1.0; N[KG_BROKE] = S[KG_BROKE];
  }
}

// ---- end of a visit -------------------------------------------------------------------------------------------------------------------------
template <int METHOD, class LV> __global__ void __launch_bounds__(1024) kg_xsum(LV lv, KrylovGridArgs K) {
  constexpr int NW = (METHOD == VDN_KRYLOV_CG) ? 4 : 7;
  const int np = lv.count();
  const double *x = lv.x(), *dinv = K.w + (NW - 1) * lv.size();
  double sx[1] = { 0.0 }, m1[1] = { 0.0 };
  KG_POINTS(t, np) {
    long c; int i, j, k;
    lv.point(t, c, i, j, k);
    if (dinv[c] != 0.0) sx[0] = sx[0] + x[c];
  }
  wg_reduce<1, 0>(sx, m1);
  kg_put(K, KG_X, sx[0]);
}
template <int METHOD, class LV> __global__ void __launch_bounds__(1024) kg_finish(LV lv, KrylovGridArgs K, int cur) {
  constexpr int NW = (METHOD == VDN_KRYLOV_CG) ? 4 : 7;
  const double *S = K.st(cur);
  const double nunk = S[KG_NUNK];
  if (lv.singular() && nunk > 0.0) {
    const double xm = kg_sum(kg_part(K, KG_X), gridDim.x) / nunk;
    if (kry_finite(xm)) {
      const int np = lv.count();
      double *x = lv.x();
      const double *dinv = K.w + (NW - 1) * lv.size();
      KG_POINTS(t, np) {
        long c; int i, j, k;
        lv.point(t, c, i, j, k);
        if (dinv[c] != 0.0) x[c] = x[c] - xm;
      }
    }
  }
  if (kg_first()) {
    const double it = S[KG_IT];
    double broke = S[KG_BROKE];
    bool done = S[KG_DONE] != 0.0;
    if (METHOD == VDN_KRYLOV_BICGSTAB && !done && S[KG_PEND] != 0.0) {      // the last launched iteration's residual was never looked at
      const double rn = kg_max(kg_part(K, KG_E1), gridDim.x);
      if (!kry_finite(rn)) { broke = broke + 1.0; done = true; }
      else if (rn <= S[KG_TOL] || it >= (double)K.maxit) done = true;
    }
    K.stats[0] = K.stats[0] + 1.0;
    K.stats[1] = K.stats[1] + it;
    if (it > K.stats[2]) K.stats[2] = it;
    K.stats[3] = K.stats[3] + broke;
    if (!done) K.exhausted[0] = K.exhausted[0] + 1.0;
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
// workgroups and threads per workgroup for np points: from np alone
static inline int krylov_grid_shape(long np, int &threads) {
  threads = 256;
  if ((np + threads - 1) / threads > KG_MAXWG) threads = 512;
  if ((np + threads - 1) / threads > KG_MAXWG) threads = 1024;
  const long g = (np + threads - 1) / threads;
  return (int)(g > KG_MAXWG ? KG_MAXWG : (g < 1 ? 1 : g));
}
// one bottom visit: `budget` iterations (<= K.maxit) as plain launches on s.  The shapes come from the adapter: the fill's launch from the fill's own count
template <int METHOD, class LV> static void krylov_grid_visit(const LV &lv, const KrylovGridArgs &K, int budget, hipStream_t s) {
  constexpr int NW = (METHOD == VDN_KRYLOV_CG) ? 4 : 7;
  const long sz = lv.size(), np = lv.count(), nfill = lv.fill_count();
  const bool singular = lv.singular();
  int th; const int g = krylov_grid_shape(np, th);
  const dim3 G((unsigned)g), B((unsigned)th);
  const dim3 GF((unsigned)std::max(1L, std::min((long)KG_MAXWG, (nfill + 255) / 256))), BF(256);
  HIPCHK(hipMemsetAsync(K.w, 0, sizeof(double) * NW * sz, s));
  hipLaunchKernelGGL((kg_init0<METHOD, LV>), G, B, 0, s, lv, K);
  hipLaunchKernelGGL((kg_init1<METHOD, LV>), G, B, 0, s, lv, K);
  hipLaunchKernelGGL(kg_start, dim3(1), dim3(64), 0, s, K, g, singular ? 1 : 0);
  for (int k = 0; k < budget; k++) {
    const int cur = k & 1;
    if (METHOD == VDN_KRYLOV_CG) {
      if (nfill) hipLaunchKernelGGL((kg_fill<LV>), GF, BF, 0, s, lv, K, 1, cur);
      hipLaunchKernelGGL((kg_cg_apply<LV>), G, B, 0, s, lv, K, cur);
      hipLaunchKernelGGL((kg_cg_update<LV>), G, B, 0, s, lv, K, cur);
      hipLaunchKernelGGL((kg_cg_dir<LV>), G, B, 0, s, lv, K, cur);
    } else {
      hipLaunchKernelGGL((kg_bi_dir<LV>), G, B, 0, s, lv, K, cur);
      if (nfill) hipLaunchKernelGGL((kg_fill<LV>), GF, BF, 0, s, lv, K, 5, cur);
      hipLaunchKernelGGL((kg_bi_apply<0, LV>), G, B, 0, s, lv, K, cur);
      hipLaunchKernelGGL((kg_bi_half<LV>), G, B, 0, s, lv, K, cur);
      if (nfill) hipLaunchKernelGGL((kg_fill<LV>), GF, BF, 0, s, lv, K, 5, cur);
      hipLaunchKernelGGL((kg_bi_apply<1, LV>), G, B, 0, s, lv, K, cur);
      hipLaunchKernelGGL((kg_bi_full<LV>), G, B, 0, s, lv, K, cur);
    }
  }
  if (singular) hipLaunchKernelGGL((kg_xsum<METHOD, LV>), G, B, 0, s, lv, K);
  hipLaunchKernelGGL((kg_finish<METHOD, LV>), G, B, 0, s, lv, K, budget & 1);
  if (nfill) hipLaunchKernelGGL((kg_fill<LV>), GF, BF, 0, s, lv, K, -1, -1);
}
// what wg_krylov takes of a hierarchy's solver, for multigrid `which` (0 cell-centred, 1 nodal) with its tolerance eps (mg_krylov_visit; the tail-cycle launches)
inline KrylovArgs mg_krylov_args(const MgKrylov &kry, int which, double eps) { return KrylovArgs{ kry.w, bottom_stats_dev(which), eps, kry.maxit }; }
// One visit of the bottom level `lv` adapts by the Krylov solver the hierarchy selected: one workgroup, or -- kry.part set by mg_krylov_setup -- the whole GPU
template <class LV> void mg_krylov_visit(const MgKrylov &kry, int which, double eps, const LV &lv) {
  hipStream_t s = ctx().stream;
  if (!kry.part) { hipLaunchKernelGGL((kk_bottom_krylov<LV>), dim3(1), dim3(1024), 0, s, lv, mg_krylov_args(kry, which, eps), kry.method); return; }
  const KrylovGridArgs K{ kry.w, kry.part, bottom_stats_dev(which), bottom_exhausted_dev(which), eps, kry.maxit };
  if (kry.method == VDN_KRYLOV_CG) krylov_grid_visit<VDN_KRYLOV_CG>(lv, K, kry.budget, s);
  else krylov_grid_visit<VDN_KRYLOV_BICGSTAB>(lv, K, kry.budget, s);
}
