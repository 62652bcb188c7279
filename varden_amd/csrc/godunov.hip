// godunov.hip -- unsplit Godunov predictors on CDNA4: limited slopes, MAC-velocity prediction
// (velpred) and edge states / fluxes (mkflux).
//
// Reference arithmetic restated (expression order kept; built with -ffp-contract=off):
//   slopes   src/slope.f90:148-588
//   velpred  src/velpred.f90:1776-2765  (velpred_3d, the default rolling kernel, incl. its hi-x
//            OUTLET min() at :2075)
//   mkflux   src/mkflux.f90:1186-2567   (mkflux_3d)
//
// MI355X mapping (round 1): the reference marches k-planes serially with ~30 live 2-D planes.  Here
// every stage of the data-flow DAG (A slopes, B normal predictor, C transverse
// states, D edge states) is one kernel over the whole box, one thread per cell handling that cell's
// three lower faces, x fastest so each wave row is a 512-byte coalesced segment; the one-dimensional
// predictor pairs (s_L, s_R) are recomputed where needed instead of being stored (flops are free, HBM
// is not), and only the upwinded stage results (3 + 6 fields per component) travel through HBM.
// The per-box dead-band eps needs a max-reduction: wave shuffles + one atomic per wave, consumed from
// device memory by the next kernel (no host round trip).
#include "vdn_dev.h"
#include "slopes_plan.h"
#include "godunov_plan.h"
#include <algorithm>
#include <type_traits>

// ---------------------------------------------------------------------------------------------------
struct GArgs {
  int lo[3], hi[3];
  int phys[3][2];
  int adv[3][2][3];          // adv bc of the (up to 3) advected components, for the slope specials
  double dx[3], dt;
  int ncomp, is_vel, use_minion, slope_order;
  int cons[3];
  int outlet2d;              // 1: velpred's hi-x OUTLET takes velpred_2d's rule (max, velpred.f90:305) instead of velpred_3d's (min, :2075): vdn_set_extruded_2d
};

template <int D> DEVI double ld(const FV &f, int i, int j, int k, int off, int c = 0) {
  return fv_get(f, i + (D == 0 ? off : 0), j + (D == 1 ? off : 0), k + (D == 2 ? off : 0), c);
}
template <int D> DEVI int coord(int i, int j, int k) { return D == 0 ? i : (D == 1 ? j : k); }
DEVI double sgn1(double x) { return copysign(1.0, x); }

// ---- stage A: slopes --------------------------------------------------------------------------------
struct Fromm { double cen, lim, flag, fromm; };
DEVI Fromm fromm_of(double sm, double s0, double sp) {     // slope.f90:226-235
  Fromm f;
  f.cen = 0.5 * (sp - sm);
  double dmin = 2.0 * (s0 - sm), dpls = 2.0 * (sp - s0);
  double l = fmin(fabs(dmin), fabs(dpls));
  f.lim = (dpls * dmin > 0.0) ? l : 0.0;
  f.flag = sgn1(f.cen);
  f.fromm = f.flag * fmin(f.lim, fabs(f.cen));
  return f;
}
DEVI double limited(double del, double sm, double s0, double sp) {   // the one-sided boundary slope limiter
  double dmin = 2.0 * (s0 - sm), dpls = 2.0 * (sp - s0);
  double slim = fmin(fabs(dpls), fabs(dmin));
  slim = (dpls * dmin > 0.0) ? slim : 0.0;
  return sgn1(del) * fmin(slim, fabs(del));
}

// the limited slope of a cell from its five values along one direction (m2 .. p2 = offsets -2 .. +2); pos: the cell's index along that
// direction, is / ie: first / last valid index, lo_sp / hi_sp: EXT_DIR or HOEXTRAP on that face (the one-sided formulas of slope.f90)
DEVI double slope_vals(double m2, double m1, double s0, double p1, double p2, int pos, int is, int ie, bool lo_sp, bool hi_sp, int order) {
  if (order == 0) return 0.0;
  const double two3rd = 2.0 / 3.0, sixth = 1.0 / 6.0, third = 1.0 / 3.0, tenth = 0.1;
  if (lo_sp && pos == is - 1) return 0.0;
  if (hi_sp && pos == ie + 1) return 0.0;
  if (order == 2) {
    if (lo_sp && pos == is) return limited((p1 + 3.0 * s0 - 4.0 * m1) * third, m1, s0, p1);      // slope.f90:192-199
    if (hi_sp && pos == ie) return limited(-(m1 + 3.0 * s0 - 4.0 * p1) * third, m1, s0, p1);     // slope.f90:205-213
    return limited(0.5 * (p1 - m1), m1, s0, p1);                                                  // 181-187
  }
  // 4th order
  if (lo_sp && pos == is) return limited(-16.0 / 15.0 * m1 + 0.5 * s0 + two3rd * p1 - tenth * p2, m1, s0, p1);       // 247-254
  if (hi_sp && pos == ie) return limited(-(-16.0 / 15.0 * p1 + 0.5 * s0 + two3rd * m1 - tenth * m2), m1, s0, p1);    // 268-275
  Fromm f0 = fromm_of(m1, s0, p1);
  double fp, fm;
  if (hi_sp && pos == ie - 1)       // revised fromm(ie) = slope(ie)   (slope.f90:277-281)
    fp = limited(-(-16.0 / 15.0 * p2 + 0.5 * p1 + two3rd * s0 - tenth * m1), s0, p1, p2);
  else fp = fromm_of(s0, p1, p2).fromm;          // fromm(i+1) uses s(i), s(i+1), s(i+2)
  if (lo_sp && pos == is + 1)       // revised fromm(is) = slope(is)   (slope.f90:256-260)
    fm = limited(-16.0 / 15.0 * m2 + 0.5 * m1 + two3rd * s0 - tenth * p1, m2, m1, s0);
  else
    fm = fromm_of(m2, m1, s0).fromm;
  double ds = 2.0 * two3rd * f0.cen - sixth * (fp + fm);
  return f0.flag * fmin(fabs(ds), f0.lim);
}
// slope of component c along D at cell (i,j,k); needs s at offsets -2..+2 along D
template <int D> DEVI double slope_at(const FV &s, int c, int i, int j, int k, int is, int ie, bool lo_sp, bool hi_sp, int order) {
  if (order == 0) return 0.0;
  const double m2 = ld<D>(s, i, j, k, -2, c), m1 = ld<D>(s, i, j, k, -1, c), s0 = ld<D>(s, i, j, k, 0, c),
               p1 = ld<D>(s, i, j, k, 1, c), p2 = ld<D>(s, i, j, k, 2, c);
  return slope_vals(m2, m1, s0, p1, p2, coord<D>(i, j, k), is, ie, lo_sp, hi_sp, order);
}

DEVI void slopes_cell(const FV &s, const FV &sl0, const FV &sl1, const FV &sl2, const GArgs &A, int dirmask, int i, int j, int k) {
  for (int c = 0; c < A.ncomp; c++) {
    #define SPEC(d, sd) (A.adv[d][sd][c] == VDN_EXT_DIR || A.adv[d][sd][c] == VDN_HOEXTRAP)
    if (dirmask & 1) fv_at(sl0, i, j, k, c) = slope_at<0>(s, c, i, j, k, A.lo[0], A.hi[0], SPEC(0, 0), SPEC(0, 1), A.slope_order);
    if (dirmask & 2) fv_at(sl1, i, j, k, c) = slope_at<1>(s, c, i, j, k, A.lo[1], A.hi[1], SPEC(1, 0), SPEC(1, 1), A.slope_order);
    if (dirmask & 4) fv_at(sl2, i, j, k, c) = slope_at<2>(s, c, i, j, k, A.lo[2], A.hi[2], SPEC(2, 0), SPEC(2, 1), A.slope_order);
    #undef SPEC
  }
}
// vmax (velpred only): max |u| over the valid cells of the three components rides along (kk_velmax, velpred.f90:1965-1975) -- the
// kernel reads every cell of u anyway
__global__ void __launch_bounds__(256) kk_slopes(FV s, FV sl0, FV sl1, FV sl2, GArgs A, Range3 r, int dirmask, double *vmax = nullptr) {
  THREAD_IJK(r)
  if (in_range) slopes_cell(s, sl0, sl1, sl2, A, dirmask, i, j, k);
  if (vmax) {                                     // uniform
    double m = 0.0;
    if (in_range && i >= A.lo[0] && i <= A.hi[0] && j >= A.lo[1] && j <= A.hi[1] && k >= A.lo[2] && k <= A.hi[2])
      m = fmax(m, fmax(fmax(fabs(fv_get(s, i, j, k, 0)), fabs(fv_get(s, i, j, k, 1))), fabs(fv_get(s, i, j, k, 2))));
    block_atomic_max(vmax, m);
  }
}

// k-marching form of kk_slopes for all three directions at once: kk_slopes reads the five values of every direction through the L1 (13
// loads per cell and component; texture addresser busy 73 %, 2.1 GB fetched for 0.43 GB of s).  Here a thread keeps the five planes
// k-2 .. k+2 of its column in registers (one load per plane and component) and takes x-neighbours from the lanes next to it; the y-neighbours
// of plane k come straight from memory (they are the values the rows next door loaded two planes ago: L2 hits), so there is no LDS, no barrier
// and no row overlap -- 64 x 4 threads own 60 x 4 cells, several workgroups share a CU.  slope_vals on the same values.
// (Counters: 1.77 GB fetched per three-component launch for 0.43 GB of s -- the row and plane halos of neighbouring tiles rarely meet in one L2.  Measured and not
// kept: the XCD-aware tile order of the other marches (xcd_tile) 0.645 -> 0.674 ms, with 64 x 8 workgroups 0.87 ms; fewer k-chunks no better.)
// (Measured on this form and not kept: one fromm_of per cell along x and z -- the neighbours' from the lanes next door / carried from plane to plane -- instead of
// three: 0.659 -> 0.737 ms for three components, 0.390 -> 0.412 for two; the kernel is not bound by its arithmetic.)
// (Re-measured before the pair form below replaced it as the default: 0.667 / 0.413 ms per launch for three / two components at 256^3, 1.73 / 1.13 GB fetched for 0.43 / 0.29 GB of s,
// the texture addresser busy 70 % of the kernel's cycles -- profiles/slopes_march_ab.txt.  It stays for boxes of odd width and misaligned arrays, and as VDN_SLOPES_MARCH=1.)
template <int NC> __global__ void __launch_bounds__(256) kk_slopes_my(FV s, FV sl0, FV sl1, FV sl2, GArgs A, Range3 r, int klen, double *vmax) {
  const int lane = threadIdx.x, row = threadIdx.y;
  const int i = r.lo[0] - 2 + (int)blockIdx.x * 60 + lane, j = r.lo[1] + (int)blockIdx.y * 4 + row;
  const bool own_ij = lane >= 2 && lane <= 61 && i <= r.hi[0] && j <= r.hi[1];
  const int ic = min(max(i, A.lo[0] - 3), A.hi[0] + 3), jc = min(max(j, A.lo[1] - 3), A.hi[1] + 3);
  const int k0 = r.lo[2] + (int)blockIdx.z * klen, k1 = min(k0 + klen - 1, r.hi[2]);
  const long sp = (long)s.n0 * s.n1;
  long oy[4];                                                         // rows j-2, j-1, j+1, j+2 relative to the column (kept inside the allocation like the planes)
  { const int dj[4] = { -2, -1, 1, 2 };
    #pragma unroll
    for (int q = 0; q < 4; q++) oy[q] = (long)(min(max(j + dj[q], A.lo[1] - 3), A.hi[1] + 3) - jc) * s.n0; }
  const double *ps[NC];
  #pragma unroll
  for (int c = 0; c < NC; c++) ps[c] = s.p + fv_idx(s, ic, jc, s.a2) + s.sc * c;
  #define SPL(c, kk) ps[c][(long)(min(max((kk), A.lo[2] - 3), A.hi[2] + 3) - s.a2) * sp]
  #define SPY(c, kk, q) ps[c][(long)(min(max((kk), A.lo[2] - 3), A.hi[2] + 3) - s.a2) * sp + oy[q]]
  #define SPEC(d, sd, c) (A.adv[d][sd][c] == VDN_EXT_DIR || A.adv[d][sd][c] == VDN_HOEXTRAP)
  double w[NC][5];
  #pragma unroll
  for (int c = 0; c < NC; c++) { w[c][0] = 0.0; for (int q = 1; q < 5; q++) w[c][q] = SPL(c, k0 - 3 + q); }
  double m = 0.0;
  for (int k = k0; k <= k1; k++) {
    double y[NC][4];
    #pragma unroll
    for (int c = 0; c < NC; c++) {
      w[c][0] = w[c][1]; w[c][1] = w[c][2]; w[c][2] = w[c][3]; w[c][3] = w[c][4]; w[c][4] = SPL(c, k + 2);
      #pragma unroll
      for (int q = 0; q < 4; q++) y[c][q] = SPY(c, k, q);
    }
    #pragma unroll
    for (int c = 0; c < NC; c++) {
      const double s0 = w[c][2];
      const double xm1 = lane_prev(s0), xp1 = lane_next(s0), xm2 = lane_prev(xm1), xp2 = lane_next(xp1);
      if (own_ij) {
        fv_at(sl0, i, j, k, c) = slope_vals(xm2, xm1, s0, xp1, xp2, i, A.lo[0], A.hi[0], SPEC(0, 0, c), SPEC(0, 1, c), A.slope_order);
        fv_at(sl2, i, j, k, c) = slope_vals(w[c][0], w[c][1], s0, w[c][3], w[c][4], k, A.lo[2], A.hi[2], SPEC(2, 0, c), SPEC(2, 1, c), A.slope_order);
        fv_at(sl1, i, j, k, c) = slope_vals(y[c][0], y[c][1], s0, y[c][2], y[c][3], j, A.lo[1], A.hi[1], SPEC(1, 0, c), SPEC(1, 1, c), A.slope_order);
      }
      if (own_ij && vmax && i >= A.lo[0] && i <= A.hi[0] && j >= A.lo[1] && j <= A.hi[1] && k >= A.lo[2] && k <= A.hi[2]) m = fmax(m, fabs(s0));
    }
  }
  #undef SPL
  #undef SPY
  #undef SPEC
  if (vmax) block_atomic_max(vmax, m);
}
// Pair form of the march above (slopes_plan.h): a lane owns the cells (i, i + 1) and moves them as 16-byte values -- per pair and component 1 + 1/2 loads and
// 3 stores where kk_slopes_my issues 10 and 6.  Five planes of the pair's column stay in registers, the plane after them is loaded one iteration ahead; the
// x-neighbours are the two values of the lanes next door.  Each y-neighbour is fetched once: the workgroup (SLP_WAVES waves, one full-width row or 64 >> lw
// narrow ones each) stages plane k of its rows and of two halo rows either side in LDS -- own rows from the registers, the halo rows loaded one plane ahead by
// the first 4 * 2^lw threads -- double-buffered, one barrier per plane, and reads the rows j - 2, j - 1, j + 1, j + 2 from there.  The last pairs of a row that
// fill no 62-pair segment march in narrow segments of the same launch (a 258-cell row: two full segments and 5 pairs in 8-lane segments, 64 rows per
// workgroup).  slope_vals on the same values: the same bits.  Loads are clamped into the box grown by three, pairwise: no lane leaves the allocation.
// A workgroup marches ONE component (blockIdx.z): the components share nothing but max |u|, and three of them in one thread are 162 VGPRs, 107 spilled SGPRs
// and 64 bytes of scratch (the lane masks of slope_vals' position tests for two cells, three components, two directions); one is 97 VGPRs, no scratch, 24 KB
// of LDS, two workgroups per CU.
// (Measured at 256^3, three / two components, per launch: kk_slopes_my 0.667 / 0.413 ms; pairs alone, the y-neighbours still from memory: 0.537 / 0.332 with
// four waves, 0.547 / 0.352 with eight; with the rows staged: 0.476 / 0.318, four waves 0.474 / 0.309, sixteen 0.593 / 0.411.  Eight are kept: they stage 12
// rows for 8 where four stage 8 for 4.  Workgroups per component (SLP_WG_TARGET) 512: 0.486 / 0.349, 1024: 0.475 / 0.320, 2048: 0.480 / 0.325, 4096: 0.477 / 0.315.)
template <int NC> __global__ void __launch_bounds__(64 * SLP_WAVES) kk_slopes_pr(FV s, FV sl0, FV sl1, FV sl2, GArgs A, Range3 r, SlopesPlan P, double *vmax) {
  __shared__ double2 sm[2][(SLP_WAVES + 4) * 64];
  const int tid = threadIdx.x, c = blockIdx.z;                       // grid: tiles x k-chunks x NC components
  int lw, pair0, by, pl, rr, hrow, hslot;
  slopes_tile(P, (int)blockIdx.x, lw, pair0, by);
  const bool own_l = slopes_lane(lw, tid, pl, rr), hal = slopes_halo(lw, tid, hrow, hslot);
  const int W = 1 << lw, j0 = r.lo[1] + by * (SLP_WAVES * (64 >> lw));
  const int i_ = r.lo[0] + 2 * (pair0 + pl - 1), j_ = j0 + rr;
  const bool own = own_l && i_ <= r.hi[0] && j_ <= r.hi[1];
  const int ic = min(max(i_, A.lo[0] - 3), A.hi[0] + 2), jc = min(max(j_, A.lo[1] - 3), A.hi[1] + 3), jh = min(max(j0 + hrow, A.lo[1] - 3), A.hi[1] + 3);
  const int k0 = r.lo[2] + (int)blockIdx.y * P.klen, k1 = min(k0 + P.klen - 1, r.hi[2]);
  const long sp = (long)s.n0 * s.n1, slp = (long)sl0.n0 * sl0.n1;
  const double *pw = s.p + s.sc * c + fv_idx(s, ic, jc, s.a2), *ph = s.p + s.sc * c + fv_idx(s, ic, hal ? jh : jc, s.a2);
  const long so = fv_idx(sl0, own ? i_ : r.lo[0], own ? j_ : r.lo[1], sl0.a2) + sl0.sc * c;         // sl0, sl1, sl2: one layout (launch_slopes)
  #define SPL(p, kk) (*(const double2 *)((p) + (long)(min(max((kk), A.lo[2] - 3), A.hi[2] + 3) - s.a2) * sp))
  #define SPEC(d, sd) (A.adv[d][sd][c] == VDN_EXT_DIR || A.adv[d][sd][c] == VDN_HOEXTRAP)
  const bool xl = SPEC(0, 0), xh = SPEC(0, 1), yl = SPEC(1, 0), yh = SPEC(1, 1), zl = SPEC(2, 0), zh = SPEC(2, 1);
  const int o = A.slope_order;
  double2 w[5], nx, hv;
  w[0] = make_double2(0.0, 0.0);
  #pragma unroll
  for (int q = 1; q < 5; q++) w[q] = SPL(pw, k0 - 3 + q);
  nx = SPL(pw, k0 + 2);
  hv = SPL(ph, k0);
  const int o0 = (rr + 2) * W + pl, oh = hslot * W + pl;
  double m = 0.0;
  int b = 0;
  for (int k = k0; k <= k1; k++, b ^= 1) {
    w[0] = w[1]; w[1] = w[2]; w[2] = w[3]; w[3] = w[4]; w[4] = nx;
    sm[b][o0] = w[2];
    if (hal) sm[b][oh] = hv;
    nx = SPL(pw, k + 3);
    if (hal) hv = SPL(ph, k + 1);
    __syncthreads();
    const double2 s0 = w[2];
    const double2 y0 = sm[b][o0 - 2 * W], y1 = sm[b][o0 - W], y2 = sm[b][o0 + W], y3 = sm[b][o0 + 2 * W];
    const double pa = lane_prev(s0.x), pb = lane_prev(s0.y), na = lane_next(s0.x), nb = lane_next(s0.y);
    if (own) {
      const int i = i_, j = j_;
      double2 d0, d1, d2;
      d0.x = slope_vals(pa, pb, s0.x, s0.y, na, i, A.lo[0], A.hi[0], xl, xh, o);
      d0.y = slope_vals(pb, s0.x, s0.y, na, nb, i + 1, A.lo[0], A.hi[0], xl, xh, o);
      d2.x = slope_vals(w[0].x, w[1].x, s0.x, w[3].x, w[4].x, k, A.lo[2], A.hi[2], zl, zh, o);
      d2.y = slope_vals(w[0].y, w[1].y, s0.y, w[3].y, w[4].y, k, A.lo[2], A.hi[2], zl, zh, o);
      d1.x = slope_vals(y0.x, y1.x, s0.x, y2.x, y3.x, j, A.lo[1], A.hi[1], yl, yh, o);
      d1.y = slope_vals(y0.y, y1.y, s0.y, y2.y, y3.y, j, A.lo[1], A.hi[1], yl, yh, o);
      const long oc = so + (long)(k - sl0.a2) * slp;
      *(double2 *)(sl0.p + oc) = d0; *(double2 *)(sl2.p + oc) = d2; *(double2 *)(sl1.p + oc) = d1;
      if (vmax && j >= A.lo[1] && j <= A.hi[1] && k >= A.lo[2] && k <= A.hi[2]) {
        if (i >= A.lo[0] && i <= A.hi[0]) m = fmax(m, fabs(s0.x));
        if (i + 1 >= A.lo[0] && i + 1 <= A.hi[0]) m = fmax(m, fabs(s0.y));
      }
    }
  }
  #undef SPL
  #undef SPEC
  if (vmax) block_atomic_max(vmax, m);
}
// testing build (vdn_last_slopes_form): the form the last slope launch took -- 0: kk_slopes, one thread per cell; 1: kk_slopes_my; 2: kk_slopes_pr
static int g_slopes_form = 0;
int slopes_last_form() { return g_slopes_form; }
// whether a box's arrays take the pair form: the range is the box grown by one, its width even, every 16-byte access aligned (slopes_pair_ok) and the
// three slope arrays of one layout
static bool slopes_pair_fits(const FV &s, const FV sl[3], const GArgs &A, const Range3 &rg) {
  for (int d = 0; d < 3; d++) {
    if (rg.lo[d] != A.lo[d] - 1 || rg.hi[d] != A.hi[d] + 1) return false;
    const int a = d == 0 ? s.a0 : d == 1 ? s.a1 : s.a2, n = d == 0 ? s.n0 : d == 1 ? s.n1 : s.n2;
    const int b = d == 0 ? sl[0].a0 : d == 1 ? sl[0].a1 : sl[0].a2, nb = d == 0 ? sl[0].n0 : d == 1 ? sl[0].n1 : sl[0].n2;
    if (a > A.lo[d] - 3 || a + n - 1 < A.hi[d] + 3 || b > rg.lo[d] || b + nb - 1 < rg.hi[d]) return false;
  }
  const SlopesLayout Ls = { (long)rg.lo[0] - s.a0, s.n0, s.sc, (uintptr_t)s.p };
  for (int d = 0; d < 3; d++) {
    if (sl[d].a0 != sl[0].a0 || sl[d].a1 != sl[0].a1 || sl[d].a2 != sl[0].a2 || sl[d].n0 != sl[0].n0 || sl[d].n1 != sl[0].n1 || sl[d].sc != sl[0].sc) return false;
    const SlopesLayout Ll = { (long)rg.lo[0] - sl[d].a0, sl[d].n0, sl[d].sc, (uintptr_t)sl[d].p };
    if (!slopes_pair_ok(rg.hi[0] - rg.lo[0] + 1, rg.lo[0] - (A.lo[0] - 3), A.hi[0] + 3 - rg.hi[0], Ls, Ll)) return false;
  }
  return true;
}
static void launch_slopes(const FV &s, const FV sl[3], const GArgs &A, const Range3 &rg, int ncomp, double *vmax, hipStream_t st) {
  if (sw().slopes_march && (ncomp == 2 || ncomp == 3) && s.a0 <= A.lo[0] - 3 && s.a1 <= A.lo[1] - 3 && s.a2 <= A.lo[2] - 3) {
    const int nx = rg.hi[0] - rg.lo[0] + 1, ny = rg.hi[1] - rg.lo[1] + 1, nz = rg.hi[2] - rg.lo[2] + 1;
    if (sw().slopes_march >= 2 && slopes_pair_fits(s, sl, A, rg)) {
      const SlopesPlan P = slopes_plan(nx, ny, nz);
      const dim3 g(P.tiles, P.chunks, ncomp), blk(64 * SLP_WAVES, 1, 1);
      if (ncomp == 3) hipLaunchKernelGGL(kk_slopes_pr<3>, g, blk, 0, st, s, sl[0], sl[1], sl[2], A, rg, P, vmax);
      else hipLaunchKernelGGL(kk_slopes_pr<2>, g, blk, 0, st, s, sl[0], sl[1], sl[2], A, rg, P, vmax);
      g_slopes_form = 2;
      return;
    }
    g_slopes_form = 1;
    const int tiles = ((nx + 59) / 60) * ((ny + 3) / 4);
    int chunks = std::max(1, std::min(nz / 8, (32 * 256 + tiles - 1) / tiles));      // (measured at 256^3, three / two components: 4 x 256 workgroups 0.741 / 0.477 ms, 8 x 0.667 / 0.418, 16 x 0.661 / 0.406, 32 x 0.645 / 0.384)
    const int klen = (nz + chunks - 1) / chunks;
    const dim3 g((nx + 59) / 60, (ny + 3) / 4, (nz + klen - 1) / klen), blk(64, 4, 1);
    if (ncomp == 3) hipLaunchKernelGGL(kk_slopes_my<3>, g, blk, 0, st, s, sl[0], sl[1], sl[2], A, rg, klen, vmax);
    else hipLaunchKernelGGL(kk_slopes_my<2>, g, blk, 0, st, s, sl[0], sl[1], sl[2], A, rg, klen, vmax);
    return;
  }
  g_slopes_form = 0;
  hipLaunchKernelGGL(kk_slopes, grid_for(rg), dim3(64, 4, 1), 0, st, s, sl[0], sl[1], sl[2], A, rg, 7, vmax);
}

// ---- boundary rule for a (left,right) pair on a domain face (velpred.f90:2044-2079, 2200-2224;
//      mkflux.f90:1463-1515, ...) ------------------------------------------------------------------------
DEVI void bc_pair(double &L, double &R, int phys, int side, bool is_vel, bool normal, double ghost, bool quirk) {
  if (phys == VDN_INLET) { L = ghost; R = ghost; }
  else if (phys == VDN_SLIP_WALL) {
    if (is_vel && normal) { L = 0.0; R = 0.0; }
    else if (side == 0) L = R; else R = L;
  } else if (phys == VDN_NO_SLIP_WALL) {
    if (is_vel) { L = 0.0; R = 0.0; }
    else if (side == 0) L = R; else R = L;
  } else if (phys == VDN_OUTLET) {
    if (is_vel && normal) {
      double v;
      if (side == 0) v = fmin(R, 0.0);
      else v = quirk ? fmin(L, 0.0) : fmax(L, 0.0);
      L = v; R = v;
    } else if (side == 0) L = R; else R = L;
  }
}
template <int D> DEVI int face_side(const GArgs &A, int i, int j, int k) {
  const int f = coord<D>(i, j, k);
  return f == A.lo[D] ? 0 : (f == A.hi[D] + 1 ? 1 : -1);
}
DEVI double eps_from(const double *umax_p) { double um = *umax_p; return (um == 0.0) ? 1.0e-8 : 1.0e-8 * um; }

// ====================================================================================================
// mkflux
// ====================================================================================================
DEVI double upwind_mac(double L, double R, double um, double eps) {   // mkflux.f90:1520-1522
  double v = (um > 0.0) ? L : R;
  double savg = 0.5 * (L + R);
  return (fabs(um) > eps) ? v : savg;
}

// one-dimensional predictor pair of component c on the lower D-face of cell (i,j,k), after the bc
// (mkflux.f90:1440-1515 x, 1527-1602 y, 1779-1858 z)
template <int D> DEVI void mk_pair(const GArgs &A, const FV &s, const FV &slp, const FV &mac, const FV &force, const FV &macrhs,
                                   int c, int i, int j, int k, double &L, double &R) {
  const double um = fv_get(mac, i, j, k);
  const double dt2 = 0.5 * A.dt;
  const double sl = ld<D>(s, i, j, k, -1, c), sr = fv_get(s, i, j, k, c);
  L = sl + (0.5 - dt2 * um / A.dx[D]) * ld<D>(slp, i, j, k, -1, c);
  R = sr - (0.5 + dt2 * um / A.dx[D]) * fv_get(slp, i, j, k, c);
  if (A.use_minion) {
    L = L + dt2 * ld<D>(force, i, j, k, -1, c); R = R + dt2 * fv_get(force, i, j, k, c);
    if (A.cons[c]) { L = L - dt2 * sl * ld<D>(macrhs, i, j, k, -1); R = R - dt2 * sr * fv_get(macrhs, i, j, k); }
  }
  const int side = face_side<D>(A, i, j, k);
  if (side >= 0) bc_pair(L, R, A.phys[D][side], side, A.is_vel != 0, c == D, side == 0 ? sl : sr, false);
}

// stage B: simh_D on the lower faces of cell (i,j,k);  SI has 3*ncomp comps: [D*ncomp + c]
DEVI void mk_B_cell(const FV &s, const FV &sl0, const FV &sl1, const FV &sl2, const FV &um, const FV &vm, const FV &wm, const FV &force, const FV &macrhs, const FV &SI,
                    const GArgs &A, int i, int j, int k, double eps) {
  for (int c = 0; c < A.ncomp; c++) {
    double L, R;
    if (i >= A.lo[0]) { mk_pair<0>(A, s, sl0, um, force, macrhs, c, i, j, k, L, R); fv_at(SI, i, j, k, 0 * A.ncomp + c) = upwind_mac(L, R, fv_get(um, i, j, k), eps); }
    if (j >= A.lo[1]) { mk_pair<1>(A, s, sl1, vm, force, macrhs, c, i, j, k, L, R); fv_at(SI, i, j, k, 1 * A.ncomp + c) = upwind_mac(L, R, fv_get(vm, i, j, k), eps); }
    if (k >= A.lo[2]) { mk_pair<2>(A, s, sl2, wm, force, macrhs, c, i, j, k, L, R); fv_at(SI, i, j, k, 2 * A.ncomp + c) = upwind_mac(L, R, fv_get(wm, i, j, k), eps); }
  }
}
__global__ void __launch_bounds__(256) kk_mk_B(FV s, FV sl0, FV sl1, FV sl2, FV um, FV vm, FV wm, FV force, FV macrhs, FV SI, GArgs A, Range3 r, const double *umax) {
  THREAD_IJK(r)
  if (!in_range) return;
  mk_B_cell(s, sl0, sl1, sl2, um, vm, wm, force, macrhs, SI, A, i, j, k, eps_from(umax));
}

// transverse correction of a state extrapolated from cell (ci,cj,ck) by direction T
// (mkflux.f90:1620-1626 etc.):  conservative  (dt3/hT)(simhT(+)*macT(+) - simhT*macT)
//                               convective    (dt6/hT)(macT(+)+macT)(simhT(+)-simhT)
template <int T> DEVI double trans_term(const GArgs &A, const FV &SI, int comp_idx, const FV &macT, bool cons,
                                        int ci, int cj, int ck, double fcons, double fconv) {
  const double sp = ld<T>(SI, ci, cj, ck, 1, comp_idx), s0 = fv_get(SI, ci, cj, ck, comp_idx);
  const double mp = ld<T>(macT, ci, cj, ck, 1), m0 = fv_get(macT, ci, cj, ck);
  if (cons) return (fcons / A.dx[T]) * (sp * mp - s0 * m0);
  return (fconv / A.dx[T]) * (mp + m0) * (sp - s0);
}

// stage C for one (D,T): SC[(D,T)] on the lower D-face of cell (i,j,k)
template <int D, int T> DEVI void mk_C_one(const GArgs &A, const FV &s, const FV &slp, const FV &macD, const FV &macT, const FV &force,
                                           const FV &macrhs, const FV &SI, const FV &SC, int c, int i, int j, int k, double eps) {
  constexpr int O = 3 - D - T;
  const int qd = coord<D>(i, j, k), qt = coord<T>(i, j, k);
  if (qd < A.lo[D] || qt < A.lo[T] || qt > A.hi[T]) return;       // normal faces lo..hi+1, T valid, O grown
  (void)O;
  double L, R;
  mk_pair<D>(A, s, slp, macD, force, macrhs, c, i, j, k, L, R);
  const double dt3 = A.dt / 3.0, dt6 = A.dt / 6.0;
  const int ci = i - (D == 0), cj = j - (D == 1), ck = k - (D == 2);
  L = L - trans_term<T>(A, SI, T * A.ncomp + c, macT, A.cons[c] != 0, ci, cj, ck, dt3, dt6);
  R = R - trans_term<T>(A, SI, T * A.ncomp + c, macT, A.cons[c] != 0, i, j, k, dt3, dt6);
  const int side = face_side<D>(A, i, j, k);
  if (side >= 0) bc_pair(L, R, A.phys[D][side], side, A.is_vel != 0, c == D, side == 0 ? ld<D>(s, i, j, k, -1, c) : fv_get(s, i, j, k, c), false);
  // SC component index: (D*2 + (T > D ? T-1 : T)) * ncomp + c
  fv_at(SC, i, j, k, (D * 2 + (T > D ? T - 1 : T)) * A.ncomp + c) = upwind_mac(L, R, fv_get(macD, i, j, k), eps);
}
DEVI int sc_idx(int D, int T, int ncomp, int c) { return (D * 2 + (T > D ? T - 1 : T)) * ncomp + c; }

DEVI void mk_C_cell(const FV &s, const FV &sl0, const FV &sl1, const FV &sl2, const FV &um, const FV &vm, const FV &wm, const FV &force, const FV &macrhs, const FV &SI, const FV &SC,
                    const GArgs &A, int i, int j, int k, double eps) {
  for (int c = 0; c < A.ncomp; c++) {
    mk_C_one<0, 1>(A, s, sl0, um, vm, force, macrhs, SI, SC, c, i, j, k, eps);
    mk_C_one<0, 2>(A, s, sl0, um, wm, force, macrhs, SI, SC, c, i, j, k, eps);
    mk_C_one<1, 0>(A, s, sl1, vm, um, force, macrhs, SI, SC, c, i, j, k, eps);
    mk_C_one<1, 2>(A, s, sl1, vm, wm, force, macrhs, SI, SC, c, i, j, k, eps);
    mk_C_one<2, 0>(A, s, sl2, wm, um, force, macrhs, SI, SC, c, i, j, k, eps);
    mk_C_one<2, 1>(A, s, sl2, wm, vm, force, macrhs, SI, SC, c, i, j, k, eps);
  }
}
__global__ void __launch_bounds__(256) kk_mk_C(FV s, FV sl0, FV sl1, FV sl2, FV um, FV vm, FV wm, FV force, FV macrhs, FV SI, FV SC, GArgs A, Range3 r, const double *umax) {
  THREAD_IJK(r)
  if (!in_range) return;
  mk_C_cell(s, sl0, sl1, sl2, um, vm, wm, force, macrhs, SI, SC, A, i, j, k, eps_from(umax));
}

// stage D for direction D (mkflux.f90:2307-2408 x, 2411-2511 y, 1867-1972 z)
template <int D> DEVI void mk_D_one(const GArgs &A, const FV &s, const FV &slp, const FV &macD, const FV &macT1, const FV &macT2,
                                    const FV &force, const FV &macrhs, const FV &SC, const FV &sedge, const FV &flux,
                                    int c, int i, int j, int k, double eps) {
  constexpr int T1 = (D == 0) ? 1 : 0, T2 = (D == 2) ? 1 : 2;
  if (coord<T1>(i, j, k) > A.hi[T1] || coord<T2>(i, j, k) > A.hi[T2]) return;
  double L, R;
  mk_pair<D>(A, s, slp, macD, force, macrhs, c, i, j, k, L, R);
  const double dt2 = 0.5 * A.dt, dt4 = A.dt / 4.0;
  const bool cons = A.cons[c] != 0;
  double LR[2] = { L, R };
  #pragma unroll
  for (int sd = 0; sd < 2; sd++) {
    const int ci = i - ((sd == 0) && D == 0), cj = j - ((sd == 0) && D == 1), ck = k - ((sd == 0) && D == 2);
    // the T1 term uses the T1-face state corrected by T2 (e.g. sedgex: simhyz), the T2 term the T2-face
    // state corrected by T1 (simhzy)
    double v = LR[sd];
    v = v - trans_term<T1>(A, SC, sc_idx(T1, T2, A.ncomp, c), macT1, cons, ci, cj, ck, dt2, dt4);
    v = v - trans_term<T2>(A, SC, sc_idx(T2, T1, A.ncomp, c), macT2, cons, ci, cj, ck, dt2, dt4);
    const double s0 = fv_get(s, ci, cj, ck, c);
    if (cons) {
      v = v + (dt2 / A.dx[T1]) * s0 * (ld<T1>(macT1, ci, cj, ck, 1) - fv_get(macT1, ci, cj, ck));
      v = v + (dt2 / A.dx[T2]) * s0 * (ld<T2>(macT2, ci, cj, ck, 1) - fv_get(macT2, ci, cj, ck));
    }
    if (!A.use_minion) {
      v = v + dt2 * fv_get(force, ci, cj, ck, c);
      if (cons) v = v - dt2 * s0 * fv_get(macrhs, ci, cj, ck);
    }
    LR[sd] = v;
  }
  const double um = fv_get(macD, i, j, k);
  double e = upwind_mac(LR[0], LR[1], um, eps);
  const int side = face_side<D>(A, i, j, k);
  if (side >= 0) {                                   // mkflux.f90:2369-2402
    const int ph = A.phys[D][side];
    const double in = (side == 0) ? LR[1] : LR[0];
    const bool vel = A.is_vel != 0;
    if (ph == VDN_INLET) e = (side == 0) ? ld<D>(s, i, j, k, -1, c) : fv_get(s, i, j, k, c);
    else if (ph == VDN_SLIP_WALL) e = (vel && c == D) ? 0.0 : in;
    else if (ph == VDN_NO_SLIP_WALL) e = vel ? 0.0 : in;
    else if (ph == VDN_OUTLET) e = (vel && c == D) ? ((side == 0) ? fmin(in, 0.0) : fmax(in, 0.0)) : in;
  }
  fv_at(sedge, i, j, k, c) = e;
  if (cons) fv_at(flux, i, j, k, c) = e * um;        // mkflux.f90:1969, 2405, 2508
}

DEVI void mk_D_cell(const FV &s, const FV &sl0, const FV &sl1, const FV &sl2, const FV &um, const FV &vm, const FV &wm, const FV &force, const FV &macrhs, const FV &SC,
                    const FV &sex, const FV &sey, const FV &sez, const FV &flx, const FV &fly, const FV &flz, const GArgs &A, int i, int j, int k, double eps) {
  for (int c = 0; c < A.ncomp; c++) {
    mk_D_one<0>(A, s, sl0, um, vm, wm, force, macrhs, SC, sex, flx, c, i, j, k, eps);
    mk_D_one<1>(A, s, sl1, vm, um, wm, force, macrhs, SC, sey, fly, c, i, j, k, eps);
    mk_D_one<2>(A, s, sl2, wm, um, vm, force, macrhs, SC, sez, flz, c, i, j, k, eps);
  }
}
__global__ void __launch_bounds__(256) kk_mk_D(FV s, FV sl0, FV sl1, FV sl2, FV um, FV vm, FV wm, FV force, FV macrhs, FV SC,
                        FV sex, FV sey, FV sez, FV flx, FV fly, FV flz, GArgs A, Range3 r, const double *umax) {
  THREAD_IJK(r)
  if (!in_range) return;
  mk_D_cell(s, sl0, sl1, sl2, um, vm, wm, force, macrhs, SC, sex, sey, sez, flx, fly, flz, A, i, j, k, eps_from(umax));
}


// ====================================================================================================
// Cell-centred, k-marching form of the stage B / C / D kernels (the default path)
// ====================================================================================================
// Measured on MI355X (rocprofv3 PMC, 256^3): the face-centred kernels above issue ~230 loads per cell in stage D, most of
// them re-reading, for the LEFT side of a face, what the neighbouring thread reads for the RIGHT side of its own face;
// the per-CU vector L1 (TCP) is the bound (1.1e9 tag accesses, 1.8e9 pending-stall cycles per launch), not HBM.
// Every left/right state of a face is a function of ONE cell (the cell on that side), so here a thread owns a CELL,
// computes that cell's contribution to its lower faces (right states) and to its upper faces (left states) once, and
// hands the left states to the owner of the upper face:
//   x: to lane+1 by a wave shuffle      (tiles overlap by one cell: lane 0 is halo-only)
//   y: to row+1 through LDS             (tiles overlap by one row: row 0 is halo-only, one barrier per plane)
//   z: to itself at the next k-plane    (the workgroup marches in k; a register carry)
// The arithmetic of every state is unchanged (same expressions in the same order), so results are bit-identical.
// Boundary rule: on a physical boundary face the state of the OUTSIDE cell is dead (bc_pair overwrites it from the
// inside state or the ghost value) and the inside cell can apply its half of bc_pair alone; bc_pair is idempotent, so
// the face owner then applies the complete rule to the pair it has assembled.
// Code shape: every plane starts with ONE unconditional batch of loads (indices clamped into the arrays; threads outside
// the computable region produce values nobody uses), the rare boundary work sits in one branch after it.
static bool use_batched(const vdn_multifab *s) {             // the rule and its measurements: god_use_batched
  long cells = 0;
  for (int b = 0; b < s->nfabs(); b++) cells += (long)(s->vbox[b].hi[0] - s->vbox[b].lo[0] + 1) * (s->vbox[b].hi[1] - s->vbox[b].lo[1] + 1) * (s->vbox[b].hi[2] - s->vbox[b].lo[2] + 1);
  return god_use_batched(s->nfabs(), cells, sw().godunov_batch);
}
bool god_per_box(const vdn_multifab *s) { return s->nfabs() >= 1 && !use_batched(s); }
// tile order of the marching kernels: XCD-aware (vdn_dev.h xcd_tile)
__constant__ int g_god_xcd = 1;
DEVI void xcd_remap(int &bx, int &by, int &bz) { if (g_god_xcd) xcd_tile(bx, by, bz); else { bx = blockIdx.x; by = blockIdx.y; bz = blockIdx.z; } }
DEVI double shfl_prev(double v) { return lane_prev(v); }

// ---- stages B + C + D in one march (one component per launch) ------------------------------------------------------------------
// The three stages above exchange SI (3 fields per component) and SC (6 per component) through HBM: at 256^3 the velocity mkflux moves
// 18 GB against 2.5 GB of algorithmic traffic (profiles/r02_godunov_pmc.md).  Here a workgroup keeps them in registers: iteration kk of
// the march loads plane kk and runs stage B on plane kk, stage C on plane kk-1 (its upper z-face SI is B's output of this iteration) and
// stage D on plane kk-2 (its upper z-face SC is C's output of this iteration).  A cell's upper x-face value is the next lane's lower-face
// value (DPP), its upper y-face value the next row's (LDS, written one iteration earlier), its own left states come from the previous
// lane / row / plane exactly as in the cell-centred scheme above.  A tile therefore owns lanes 1..62 and rows 1..TNY-2: the transverse couplings
// alternate direction from stage to stage, so the footprint of an output face is one cell either side, not one per stage.
// Every expression is the one of the face-centred stages (mk_pair, mk_C_one, mk_D_one) in the same order: bit-identical results
// (tests/test_kernels_gpu.py::test_mkflux, test_godunov_marching_equals_face_centred).  Reads per component: s, three slopes, three MAC
// components (+ their upper faces), force, mac_rhs; writes: three edge states (+ fluxes of conservative components).
// Memory access: the launch carries, per field, the address of plane KB = lo_z - 1 of the component (bytes) and the bytes per plane; a thread
// keeps ONE 32-bit byte offset per field layout for its (i,j) column and the workgroup advances uniform plane pointers (scalar registers)
// as the march proceeds -- no per-load index arithmetic (15 fields x fv_idx per plane cost ~150 VALU / ~180 SALU instructions per plane in
// the first version, and the 40-byte FV descriptors 170 spilled SGPRs).  The quotients of launch constants that the separate stages
// compute per cell -- dt/3/dx, dt/6/dx, ... -- are evaluated once on the host (the same IEEE operations on the same operands).
struct FGeo { int a0, a1, n0; };
struct FArgs {
  const char *p[9];       // s, sl0, sl1, sl2, um, vm, wm, force, macrhs: plane KB of the component
  long sp[7];             // bytes per plane: s, slopes, um, vm, wm, force, macrhs
  FGeo g[7];
  char *q[6];             // sex, sey, sez, flx, fly, flz
  long sq[3]; FGeo h[3];  // x-, y-, z-face outputs (edge state and flux of one direction share a layout)
  long s_row, vm_row;     // bytes per row of s / vm
  double dt2, dx[3], tC[3], tD[3], aD[3];   // tC[T] = (cons ? dt/3 : dt/6) / dx[T],  tD[T] = (cons ? dt/2 : dt/4) / dx[T],  aD[T] = (dt/2) / dx[T]
  double idx[3]; int p2;                    // 1 / dx and "every dx is a power of two": x / dx is then the exact scaling x * (1 / dx), bit for bit (P2 kernels)
  int lo[3], hi[3], phys[3][2];
  int cons, use_minion, is_vel, c;
  // UPD (round 3): update_3d of the component inside the march -- the edge states never reach memory
  char *qn; long sqn; FGeo hn;      // snew / unew of the component: plane KB, bytes per plane, layout
  const char *pfu[3]; int fmode;    // the update's forcing term: fmode 0 = the force of this call (p[7]); 1 = ext (pfu[0]) + (lapu0 - gp (pfu[1])) / rho (pfu[2]), force layout
  double dt, lapu0;
};
static bool bc_mode_host(int phys) { return phys == VDN_INLET || phys == VDN_SLIP_WALL || phys == VDN_NO_SLIP_WALL || phys == VDN_OUTLET; }
static bool same_geom(const FV &a, const FV &b) { return a.a0 == b.a0 && a.a1 == b.a1 && a.a2 == b.a2 && a.n0 == b.n0 && a.n1 == b.n1; }
DEVI unsigned fg_off(const FGeo &G, int i, int j) { return 8u * (unsigned)((i - G.a0) + G.n0 * (j - G.a1)); }
DEVI double ldd(const char *q, unsigned o) { return *(const double *)(q + o); }
DEVI void std_(char *q, unsigned o, double v) { *(double *)(q + o) = v; }
struct FCell { double m_lo[3], m_up[3], s0, f, mr, Lb[3], Rb[3]; };      // a cell's loads and its bases (before any boundary rule)
// the one-dimensional predictor bases of a cell (mk_pair split by side, no boundary rule) with the launch constants of FArgs: Lb = left state
// of the cell's upper D-face, Rb = right state of its lower D-face (force / mac_rhs terms inside only with use_minion); stages C and D of the
// face-centred kernels recompute the same ones -- six f64 divisions per cell and stage -- here they ride along with the cell
// A division by a power of two is an exact scaling: x / dx and x * (1 / dx) are the same double for every x (zeros, infinities and subnormal
// results included: both are the correctly rounded value of the same real number), so where every dx is a power of two -- the unit cube on
// 2^n cells, every level of a hierarchy over it -- the P2 kernels multiply.  The ten f64 divisions per cell and plane of the fused march were a
// third of its f64 instructions (v_div_scale x 2, v_rcp, eight fma, v_div_fmas, v_div_fixup each).  Other spacings keep the division.
static bool is_pow2(double x) { int e; return x > 0.0 && std::frexp(x, &e) == 0.5; }
#define DIVDX(x, d) (PW2 ? (x) * F.idx[d] : (x) / F.dx[d])
template <bool PW2> DEVI void f_bases(const FArgs &F, FCell &P, const double sl[3], const bool minion, const bool cons) {
  double ft = 0.0, mt = 0.0;
  if (minion) { ft = F.dt2 * P.f; mt = F.dt2 * P.s0 * P.mr; }
  #pragma unroll
  for (int d = 0; d < 3; d++) {
    double Lb = P.s0 + (0.5 - DIVDX(F.dt2 * P.m_up[d], d)) * sl[d];
    double Rb = P.s0 - (0.5 + DIVDX(F.dt2 * P.m_lo[d], d)) * sl[d];
    if (minion) {
      Lb = Lb + ft; Rb = Rb + ft;
      if (cons) { Lb = Lb - mt; Rb = Rb - mt; }
    }
    P.Lb[d] = Lb; P.Rb[d] = Rb;
  }
}
DEVI double tvq(bool cons, double q, double sp, double s0, double mp, double m0) {     // trans_term on values, its quotient (fcons / dxT or fconv / dxT) given
  if (cons) return q * (sp * mp - s0 * m0);
  return q * (mp + m0) * (sp - s0);
}
constexpr int PH_EDGE = 0, PH_STEADY = 1;   // phases of a march's plane function
// The boundary rules in compact form.  bc_pair always leaves L = R = v, and upwind_mac(v, v, .) = v, so on a physical boundary face every
// stage's output IS v -- the inflow value, zero, the inner state, or the inner state clamped (bc_pair / the edge-state rule of mk_D_one: the same four cases):
//   mode 1: ghost value   2: zero   3: inner state   4: inner state, min(.,0) on a lo face / max(.,0) on a hi face
// and the "premod" of stages C and D is the same v applied to the base of the cell next to the face.
DEVI int bc_mode(int phys, bool is_vel, bool normal) {
  if (phys == VDN_INLET) return 1;
  if (phys == VDN_SLIP_WALL) return (is_vel && normal) ? 2 : 3;
  if (phys == VDN_NO_SLIP_WALL) return is_vel ? 2 : 3;
  if (phys == VDN_OUTLET) return (is_vel && normal) ? 4 : 3;
  return 0;
}
DEVI double bc_v(int m, int side, double in, double ghost) {
  double v = in;
  if (m == 4) v = side ? fmax(in, 0.0) : fmin(in, 0.0);
  if (m == 2) v = 0.0;
  if (m == 1) v = ghost;
  return v;
}
// NAR (box-batched launches, boxes narrower than a tile): a wave carries 64 / W node... cell rows of W lanes each (lanes 1 .. W-2 of a segment own cells, the
// two outer ones feed their neighbours, exactly as lanes 0 and 63 of the full-width tile), a workgroup TNY * (64 / W) rows of which all but the first and
// last own cells; W is the descriptor's.  The shared arrays keep their size and are addressed flat (row * W + lane); lanes left over after a wave's last
// segment own nothing, load clamped addresses and park their stores in the slots the rows do not use.  A level of 997 boxes of which 670 are 8 cells wide
// marches 0.52 x the wave-planes of the full-width tiling (tools/box_histogram.py).
struct SegGeo { int W, ROWS, lane, row, rowm, rowp, o0, om, op; bool live; };
template <bool NAR, int TY = TNY> DEVI SegGeo seg_geo(int W_) {      // TY: the waves of the workgroup (THY: kk_mk_F_mh)
  SegGeo G;
  if (!NAR) {
    G.W = 64; G.ROWS = TY; G.lane = threadIdx.x; G.row = threadIdx.y; G.live = true;
    G.rowm = G.row >= 1 ? G.row - 1 : 0; G.rowp = G.row + 1 < TY ? G.row + 1 : TY - 1;
    G.o0 = G.om = G.op = 0;
    return G;
  }
  const int tid = threadIdx.x, rpw = 64 / W_;
  G.W = W_;
  GOD_THREAD_T(TY, W_, tid, (int)threadIdx.y, G.ROWS, G.live, G.lane, G.row)
  G.rowm = G.row >= 1 ? G.row - 1 : 0; G.rowp = G.row + 1 < G.ROWS ? G.row + 1 : G.ROWS - 1;
  G.o0 = G.live ? G.row * W_ + G.lane : G.ROWS * W_ + (int)threadIdx.y * (64 - rpw * W_) + (tid - rpw * W_);
  G.om = G.rowm * W_ + G.lane; G.op = G.rowp * W_ + G.lane;
  return G;
}
// this thread's slot / the slot of the row below / above in a [TNY][64] shared array
#define LS(A) (*(NAR ? &(&A[0][0])[G.o0] : &A[row][lane]))
#define LM(A) (NAR ? (&A[0][0])[G.om] : A[rowm][lane])
#define LP(A) (NAR ? (&A[0][0])[G.op] : A[rowp][lane])
// UPD: the conservative / convective update of the component (update.f90:220-269) rides along.  A cell's update needs the edge states on its
// six faces: the lower three are this thread's stage-D outputs, the upper x one the next lane's (DPP, same iteration), the upper y one the
// next row's (LDS, read one iteration later, like SI and SC), the upper z one this thread's output for the next plane.  So the x-term of
// plane k is formed with stage D of plane k, the y- and z-terms one iteration later, and seven doubles travel in between; a k-chunk runs
// one plane further (the lower z-face of its successor's first plane).  sedge and flux are not stored.  Same expressions as update_cell.
// One workgroup barrier per plane (round 5; round 4 had three).  The three stages exchange their y-direction left states through LDS (lB, lC, lD) and
// each had its own write -> barrier -> read.  What a stage WRITES depends on no LDS value of the same iteration -- stage C's lC needs t[0] (x: DPP) and
// t[2] (z: registers), stage D's lD the chain of direction y, whose transverse terms are x (DPP) and z (stage C's z-faces, registers) -- so all three
// writes move in front of one barrier, with every x- and z-direction upwind that needs no LDS value, and everything that reads LDS (this iteration's
// lB / lC / lD, last iteration's lSI / lSC / lE) behind it.  Same expressions, same operands, same bits; the buffers stay double: a wave that has
// passed barrier kk reads buffer kk & 1 and last iteration's lSI / lSC / lE while the fastest wave writes buffer (kk + 1) & 1 and this iteration's.
// the y-exchange arrays of the march, ONE allocation per kernel shared by the bodies inlined into it (boundary / lean, full-width / narrow)
template <bool UPD, int TY = TNY> struct FShared { double lB[2][TY][64], lSI[2][TY][64], lC[2][2][TY][64], lSC[2][2][TY][64], lD[2][TY][64], lE[UPD ? 2 : 1][UPD ? TY : 1][64]; };
template <bool BC, bool INL, bool UPD, bool PW2, bool NAR = false, int SP = SP_RT, bool PEEL = false, int TY = TNY> __device__ __forceinline__ void mk_F_m_body(FShared<UPD, TY> &S, const FArgs &F, const Range3 &r, int klen, const double *umax, const int BX, const int BY, const int BZ, const int segw = 64) {
  double (&lB)[2][TY][64] = S.lB, (&lSI)[2][TY][64] = S.lSI, (&lC)[2][2][TY][64] = S.lC, (&lSC)[2][2][TY][64] = S.lSC, (&lD)[2][TY][64] = S.lD;
  double (&lE)[UPD ? 2 : 1][UPD ? TY : 1][64] = S.lE;
  const SegGeo G = seg_geo<NAR, TY>(segw);
  const int lane = G.lane, row = G.row;
  const int ownx = NAR ? G.W - 2 : FNX, owny = NAR ? G.ROWS - 2 : FNY;
  GOD_CELL(r.lo, r.hi, ownx, owny, BX, BY, lane, row, G.live, i, j, own_ij)      // the tile -> cell map: godunov_plan.h
  const int ic = min(max(i, F.lo[0] - 1), F.hi[0] + 1), jc = min(max(j, F.lo[1] - 1), F.hi[1] + 1);
  const bool ing_ij = i == ic && j == jc;                            // a cell of the grown box
  const bool vx = i >= F.lo[0] && i <= F.hi[0], vy = j >= F.lo[1] && j <= F.hi[1];
  const int rowm = G.rowm, rowp = G.rowp;
  GOD_PLANES(r.lo[2], r.hi[2], klen, BZ, k0, k1)
  const int KB = F.lo[2] - 1, KT = F.hi[2] + 1;                       // the planes loads are clamped to
  const double eps = eps_from(umax);
  const bool cons = SP != SP_RT ? (SP & SP_CONS) != 0 : F.cons != 0, minion = SP != SP_RT ? (SP & SP_MINION) != 0 : F.use_minion != 0;
  const int fmode = SP != SP_RT ? ((SP & SP_FMODE1) ? 1 : 0) : F.fmode;
  // the thread's column in every field layout
  const unsigned o_s = fg_off(F.g[0], ic, jc), o_sl = fg_off(F.g[1], ic, jc), o_um = fg_off(F.g[2], ic, jc), o_vm = fg_off(F.g[3], ic, jc), o_wm = fg_off(F.g[4], ic, jc);
  const unsigned o_f = fg_off(F.g[5], ic, jc), o_mr = fg_off(F.g[6], ic, jc);
  const unsigned o_ex = fg_off(F.h[0], i, j), o_ey = fg_off(F.h[1], i, j), o_ez = fg_off(F.h[2], i, j);
  // boundary modes of this component: the face rule of the cell's lower x / y face (fm*, side fs*), the rule on the bases of the cells next
  // to a face (pm*0: lowest valid cell, its R base; pm*1: highest valid cell, its L base); z: per plane, below
  int mode[3][2];
  #pragma unroll
  for (int d = 0; d < 3; d++) { mode[d][0] = BC ? bc_mode(F.phys[d][0], F.is_vel != 0, F.c == d) : 0; mode[d][1] = BC ? bc_mode(F.phys[d][1], F.is_vel != 0, F.c == d) : 0; }
  // The rules that apply to this thread, packed into one word of 4-bit fields holding a code (0 none, 1 ghost value, 2 zero, 3 inner state,
  // 4 min(inner, 0), 5 max(inner, 0)):  field 0: the cell's lower x-face is a boundary face (+8: the hi one), 1: the cell is the lowest valid cell
  // along x (rule on its R base), 2: the highest (L base); fields 3..5: the same along y.  The z direction has the same word per plane, uniform.
  // Inside a flagged (rare, divergent) branch the code is decoded with a few selects; the word is laundered through an empty asm in every
  // stage so that the decode is not hoisted out of the march (as 64-bit masks: 186 spilled SGPRs in the first version).
  int cd[3][2];
  #pragma unroll
  for (int d = 0; d < 3; d++) { cd[d][0] = mode[d][0] == 4 ? 4 : mode[d][0]; cd[d][1] = mode[d][1] == 4 ? 5 : mode[d][1]; }
  int bcw = 0;
  if (BC) {
    if (ing_ij && i == F.lo[0]) bcw |= cd[0][0];
    if (ing_ij && i == F.hi[0] + 1 && cd[0][1]) bcw |= cd[0][1] | 8;
    if (ic == F.lo[0]) bcw |= cd[0][0] << 4;
    if (ic == F.hi[0]) bcw |= cd[0][1] << 8;
    if (ing_ij && j == F.lo[1]) bcw |= cd[1][0] << 12;
    if (ing_ij && j == F.hi[1] + 1 && cd[1][1]) bcw |= (cd[1][1] | 8) << 12;
    if (jc == F.lo[1]) bcw |= cd[1][0] << 16;
    if (jc == F.hi[1]) bcw |= cd[1][1] << 20;
  }
  // per-thread plane pointers (the thread's column in each field): inputs at the plane the next loads take (kcur), outputs at the plane stage D
  // emits next.  Fifteen uniform pointers plus their strides do not fit the scalar register file next to everything else (they were
  // spilled to VGPR lanes and read back every plane); per-thread pointers cost the one 64-bit add per load that forming the address cost anyway.
  int kcur = min(max(k0 - 2, KB), KT);
  const char *ps = F.p[0] + (long)(kcur - KB) * F.sp[0] + o_s, *psl0 = F.p[1] + (long)(kcur - KB) * F.sp[1] + o_sl, *psl1 = F.p[2] + (long)(kcur - KB) * F.sp[1] + o_sl, *psl2 = F.p[3] + (long)(kcur - KB) * F.sp[1] + o_sl;
  const char *pum = F.p[4] + (long)(kcur - KB) * F.sp[2] + o_um, *pvm = F.p[5] + (long)(kcur - KB) * F.sp[3] + o_vm, *pwm = F.p[6] + (long)(kcur - KB) * F.sp[4] + o_wm;
  const char *pf = F.p[7] + (long)(kcur - KB) * F.sp[5] + o_f, *pmr = F.p[8] + (long)(kcur - KB) * F.sp[6] + o_mr;
  char *qex = F.q[0] + (long)(k0 - KB) * F.sq[0] + o_ex, *qey = F.q[1] + (long)(k0 - KB) * F.sq[1] + o_ey, *qez = F.q[2] + (long)(k0 - KB) * F.sq[2] + o_ez;
  char *qfx = F.q[3] + (long)(k0 - KB) * F.sq[0] + o_ex, *qfy = F.q[4] + (long)(k0 - KB) * F.sq[1] + o_ey, *qfz = F.q[5] + (long)(k0 - KB) * F.sq[2] + o_ez;
  FCell P0, P1, P2;
  #define FZERO(P) { P.s0 = 0.0; P.f = 0.0; P.mr = 0.0; for (int d = 0; d < 3; d++) { P.m_lo[d] = 0.0; P.m_up[d] = 0.0; P.Lb[d] = 0.0; P.Rb[d] = 0.0; } }
  FZERO(P0) FZERO(P1)
  #undef FZERO
  double LzB = 0.0, LzC[2] = { 0.0, 0.0 }, LzD = 0.0;
  double c_tx = 0.0, c_e1 = 0.0, c_e2 = 0.0, c_vbar = 0.0, c_wbar = 0.0, c_so = 0.0, c_fu = 0.0;       // UPD: what plane k-1 hands to the next iteration
  char *qn = UPD ? F.qn + (long)(k0 - KB) * F.sqn + fg_off(F.hn, i, j) : nullptr;
  double si1[3] = { 0.0, 0.0, 0.0 };                                 // SI on the lower faces of the cell in plane kk-1
  double qp[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };                   // SC on the lower faces of the cell in plane kk-2
  // ghost values of s for the inflow rule (mode 1), read only where it applies: plane kpl, dbytes along x / y from the thread's (clamped) cell
  // (INL = false: the launch has no inflow face, the reads and their address arithmetic are compiled out)
  #define S_AT(kpl, dbytes) (INL ? ldd(ps + (long)((kpl) - kcur) * F.sp[0] + (dbytes), 0u) : 0.0)
  // v of the rule with code cd_ on the inner state `in`; the ghost value is evaluated only for the inflow rule
  #define BC_V(v, code, in, ghost_expr) { const int cd_ = (code); const double in_ = (in); double v_ = in_;                      \
      if (cd_ == 4) v_ = fmin(in_, 0.0); if (cd_ == 5) v_ = fmax(in_, 0.0); if (cd_ == 2) v_ = 0.0; if (cd_ == 1) v_ = (ghost_expr); v = v_; }
  // the face rule on the upwinded value `out` of a lower face: field sh of word w; left state L, right state Rr, this cell's s, ghost of a lo face
  #define FACE_BC(out, w, sh, L, Rr, s0_, ghost_expr) { const int f_ = ((w) >> (sh)) & 15;                                        \
      if (f_) { const bool hi_ = (f_ & 8) != 0; double o_; BC_V(o_, f_ & 7, hi_ ? (L) : (Rr), hi_ ? (s0_) : (ghost_expr)) out = o_; } }
  // the rule on the bases of the cells next to a face: fields shlo (R base of the lowest cell) and shhi (L base of the highest)
  #define PREMOD(Lb_, Rb_, w, shlo, shhi, gl_expr, gh_expr) { const int a_ = ((w) >> (shlo)) & 7; if (a_) { double o_; BC_V(o_, a_, Rb_, gl_expr) Rb_ = o_; }  \
                                                              const int b_ = ((w) >> (shhi)) & 7; if (b_) { double o_; BC_V(o_, b_, Lb_, gh_expr) Lb_ = o_; } }
  // the word of the z direction for stage plane k (clamped kc): uniform
  #define Z_WORD(k, kc) (BCP ? ((((k) == (kc) && (k) == F.lo[2]) ? cd[2][0] : 0) | (((k) == (kc) && (k) == KT && cd[2][1]) ? (cd[2][1] | 8) : 0) | \
                                (((kc) == F.lo[2]) ? cd[2][0] << 4 : 0) | (((kc) == F.hi[2]) ? cd[2][1] << 8 : 0)) : 0)
  // a plane's twelve loads are issued one iteration ahead (N): at two waves per SIMD nothing else hides their latency, and an iteration's
  // arithmetic (~500 VALU instructions per wave) is longer than the round trip
  struct FRaw { double m_lo[3], m_up[3], s0, sl[3], f, mr; } N;
  #define F_LOAD {                                                                                                \
      N.m_lo[0] = ldd(pum, 0u); N.m_up[0] = ldd(pum, 8u);                                                         \
      N.m_lo[1] = ldd(pvm, 0u); N.m_up[1] = ldd(pvm + F.vm_row, 0u);                                              \
      N.m_lo[2] = ldd(pwm, 0u); N.m_up[2] = ldd(pwm + F.sp[4], 0u);                                               \
      N.s0 = ldd(ps, 0u); N.sl[0] = ldd(psl0, 0u); N.sl[1] = ldd(psl1, 0u); N.sl[2] = ldd(psl2, 0u);               \
      N.f = ldd(pf, 0u); N.mr = ldd(pmr, 0u); }
  // move the input pointers to the (clamped) plane of march index kn
  #define F_ADVANCE(kn) { const int kc_ = min(max((kn), KB), KT);                                                 \
      if (kc_ != kcur) { ps += F.sp[0]; psl0 += F.sp[1]; psl1 += F.sp[1]; psl2 += F.sp[1]; pum += F.sp[2]; pvm += F.sp[3]; pwm += F.sp[4]; pf += F.sp[5]; pmr += F.sp[6]; kcur = kc_; } }
  F_LOAD
  F_ADVANCE(k0 - 1)
  // one plane of the march.  PH_EDGE: the warm-up and run-out conditions tested per plane; PH_STEADY: all of them known true (see the loop below);
  // bcp: with the boundary code (a body with BC may run a plane without it)
  auto plane = [&](auto ph, auto bcp, const int kk) __attribute__((always_inline)) {
    constexpr bool STEADY = decltype(ph)::value == PH_STEADY, BCP = BC && decltype(bcp)::value;
    const int buf = kk & 1;
    P2 = P1; P1 = P0;
    {
      #pragma unroll
      for (int d = 0; d < 3; d++) { P0.m_lo[d] = N.m_lo[d]; P0.m_up[d] = N.m_up[d]; }
      P0.s0 = N.s0; P0.f = N.f; P0.mr = N.mr;
      const double sl[3] = { N.sl[0], N.sl[1], N.sl[2] };
      if (STEADY || kk < k1 + 2) { F_LOAD  F_ADVANCE(kk + 2) }
      f_bases<PW2>(F, P0, sl, minion, cons);
    }
    const bool doC = STEADY || kk - 1 >= k0 - 1, doD = STEADY || kk - 2 >= k0 - 1;
    // ================= in front of the barrier: the three LDS writes and every upwind that reads no LDS value =================
    // ---- stage B, plane kk: x and z faces
    double si0[3];
    const int kB = kk, kcB = min(max(kB, KB), KT), zwB = Z_WORD(kB, kcB);
    double LxB;
    {
      LS(lB[buf]) = P0.Lb[1];
      LxB = shfl_prev(P0.Lb[0]);
      const double Lzc = LzB;
      LzB = P0.Lb[2];
      si0[0] = upwind_mac(LxB, P0.Rb[0], P0.m_lo[0], eps);
      si0[2] = upwind_mac(Lzc, P0.Rb[2], P0.m_lo[2], eps);
      if (BCP && kB == kcB) {
        int w = bcw; asm volatile("" : "+v"(w));
        if (w & 0xF) { FACE_BC(si0[0], w, 0, LxB, P0.Rb[0], P0.s0, S_AT(kcB, -8L)) }
        if ((zwB & 15) && ing_ij) { FACE_BC(si0[2], zwB, 0, Lzc, P0.Rb[2], P0.s0, P1.s0) }
      }
    }
    // ---- stage C, plane kk-1: t[0], t[2], the y left states, and the faces whose transverse term is not the y one (x-face / z term, z-face / x term)
    double qc[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    double cLb[3] = { 0.0, 0.0, 0.0 }, cRb[3] = { 0.0, 0.0, 0.0 }, ct0 = 0.0, ct2 = 0.0, cLz1 = 0.0;
    const int kC = kk - 1, kcC = min(max(kC, KB), KT), zwC = Z_WORD(kC, kcC);
    int wc = 0;
    if (doC) {
      #pragma unroll
      for (int d = 0; d < 3; d++) { cLb[d] = P1.Lb[d]; cRb[d] = P1.Rb[d]; }
      if (BCP) {
        wc = bcw; asm volatile("" : "+v"(wc));
        if (wc & 0x770770) { PREMOD(cLb[0], cRb[0], wc, 4, 8, S_AT(kcC, -8L), S_AT(kcC, 8L)) PREMOD(cLb[1], cRb[1], wc, 16, 20, S_AT(kcC, -F.s_row), S_AT(kcC, F.s_row)) }
        if (zwC & 0x770) { PREMOD(cLb[2], cRb[2], zwC, 4, 8, S_AT(kcC - 1, 0L), S_AT(kcC + 1, 0L)) }
      }
      ct0 = tvq(cons, F.tC[0], lane_next(si1[0]), si1[0], P1.m_up[0], P1.m_lo[0]);
      ct2 = tvq(cons, F.tC[2], si0[2], si1[2], P1.m_up[2], P1.m_lo[2]);
      LS(lC[buf][0]) = cLb[1] - ct0; LS(lC[buf][1]) = cLb[1] - ct2;
      const double VL01 = cLb[0] - ct2, VR01 = cRb[0] - ct2, VL20 = cLb[2] - ct0, VR20 = cRb[2] - ct0;
      const double Lx1 = shfl_prev(VL01), Lz0 = LzC[0];
      cLz1 = LzC[1];
      LzC[0] = VL20;
      qc[1] = upwind_mac(Lx1, VR01, P1.m_lo[0], eps);
      qc[4] = upwind_mac(Lz0, VR20, P1.m_lo[2], eps);
      if (BCP && kC == kcC) {
        if (wc & 0xF) { FACE_BC(qc[1], wc, 0, Lx1, VR01, P1.s0, S_AT(kcC, -8L)) }
        if ((zwC & 15) && ing_ij) { FACE_BC(qc[4], zwC, 0, Lz0, VR20, P1.s0, P2.s0) }
      }
    }
    // ---- stage D, plane kk-2: the chain of direction y (transverse terms x and z) and its left state
    double dLb[3] = { 0.0, 0.0, 0.0 }, dRb[3] = { 0.0, 0.0, 0.0 }, dVR1 = 0.0, da[3] = { 0.0, 0.0, 0.0 }, dft = 0.0, dmt = 0.0;
    const int kD = kk - 2, kcD = min(max(kD, KB), KT), zwD = Z_WORD(kD, kcD);
    int wd = 0;
    #define CHAIN1(vl_, vr_, Dd, T1, T2, q1a, q0a, q1b, q0b)                                                   \
        { const double t1 = tvq(cons, F.tD[T1], q1a, q0a, P2.m_up[T1], P2.m_lo[T1]);                             \
          const double t2 = tvq(cons, F.tD[T2], q1b, q0b, P2.m_up[T2], P2.m_lo[T2]);                             \
          double vl = dLb[Dd], vr = dRb[Dd];                                                                     \
          vl = vl - t1; vr = vr - t1; vl = vl - t2; vr = vr - t2;                                                \
          if (cons) { vl = vl + da[T1]; vr = vr + da[T1]; vl = vl + da[T2]; vr = vr + da[T2]; }                  \
          if (!minion) { vl = vl + dft; vr = vr + dft; if (cons) { vl = vl - dmt; vr = vr - dmt; } }             \
          vl_ = vl; vr_ = vr; }
    if (doD) {
      dft = F.dt2 * P2.f; dmt = F.dt2 * P2.s0 * P2.mr;
      #pragma unroll
      for (int d = 0; d < 3; d++) { dLb[d] = P2.Lb[d]; dRb[d] = P2.Rb[d]; da[d] = F.aD[d] * P2.s0 * (P2.m_up[d] - P2.m_lo[d]); }
      if (BCP) {
        wd = bcw; asm volatile("" : "+v"(wd));
        if (wd & 0x770770) { PREMOD(dLb[0], dRb[0], wd, 4, 8, S_AT(kcD, -8L), S_AT(kcD, 8L)) PREMOD(dLb[1], dRb[1], wd, 16, 20, S_AT(kcD, -F.s_row), S_AT(kcD, F.s_row)) }
        if (zwD & 0x770) { PREMOD(dLb[2], dRb[2], zwD, 4, 8, S_AT(kcD - 1, 0L), S_AT(kcD + 1, 0L)) }
      }
      double vl1;
      CHAIN1(vl1, dVR1, 1, 0, 2, lane_next(qp[1]), qp[1], qc[4], qp[4])
      LS(lD[buf]) = vl1;
    }
    __syncthreads();
    // ================= behind the barrier: everything that reads LDS =================
    // ---- stage B: the y face
    {
      const double Ly = LM(lB[buf]);
      si0[1] = upwind_mac(Ly, P0.Rb[1], P0.m_lo[1], eps);
      if (BCP && kB == kcB) {
        int w = bcw; asm volatile("" : "+v"(w));
        if (w & 0xF000) { FACE_BC(si0[1], w, 12, Ly, P0.Rb[1], P0.s0, S_AT(kcB, -F.s_row)) }
      }
      LS(lSI[buf]) = si0[1];                                   // read by the row below in the next iteration
    }
    // ---- stage C: t[1] (SI on the upper y face: the row above, last iteration) and the faces that need it or the y left states
    if (doC) {
      const double ct1 = tvq(cons, F.tC[1], LP(lSI[buf ^ 1]), si1[1], P1.m_up[1], P1.m_lo[1]);
      const double VL00 = cLb[0] - ct1, VR00 = cRb[0] - ct1, VR10 = cRb[1] - ct0, VR11 = cRb[1] - ct2, VL21 = cLb[2] - ct1, VR21 = cRb[2] - ct1;
      const double Lx0 = shfl_prev(VL00), Ly0 = LM(lC[buf][0]), Ly1 = LM(lC[buf][1]);
      LzC[1] = VL21;
      qc[0] = upwind_mac(Lx0, VR00, P1.m_lo[0], eps);
      qc[2] = upwind_mac(Ly0, VR10, P1.m_lo[1], eps); qc[3] = upwind_mac(Ly1, VR11, P1.m_lo[1], eps);
      qc[5] = upwind_mac(cLz1, VR21, P1.m_lo[2], eps);
      if (BCP && kC == kcC) {
        if (wc & 0xF00F) {
          FACE_BC(qc[0], wc, 0, Lx0, VR00, P1.s0, S_AT(kcC, -8L))
          FACE_BC(qc[2], wc, 12, Ly0, VR10, P1.s0, S_AT(kcC, -F.s_row)) FACE_BC(qc[3], wc, 12, Ly1, VR11, P1.s0, S_AT(kcC, -F.s_row))
        }
        if ((zwC & 15) && ing_ij) { FACE_BC(qc[5], zwC, 0, cLz1, VR21, P1.s0, P2.s0) }
      }
      LS(lSC[buf][0]) = qc[2]; LS(lSC[buf][1]) = qc[3];            // read by the row below in the next iteration
    }
    // ---- stage D: the chains of directions x and z, the three edge states, the update
    if (doD) {
      const int k = kD, kc = kcD, zw = zwD;
      const bool vz = k >= F.lo[2] && k <= F.hi[2];
      const double (&m_lo)[3] = P2.m_lo, (&m_up)[3] = P2.m_up;
      const double s0 = P2.s0;
      double VL[3], VR[3];
      VR[1] = dVR1;
      CHAIN1(VL[0], VR[0], 0, 1, 2, LP(lSC[buf ^ 1][1]), qp[3], qc[5], qp[5])
      CHAIN1(VL[2], VR[2], 2, 0, 1, lane_next(qp[0]), qp[0], LP(lSC[buf ^ 1][0]), qp[2])
      double L[3];
      L[0] = shfl_prev(VL[0]); L[1] = LM(lD[buf]); L[2] = LzD; LzD = VL[2];
      if (STEADY || k >= k0) {
        double e[3] = { 0.0, 0.0, 0.0 };
        if (UPD || own_ij) {
          e[0] = upwind_mac(L[0], VR[0], m_lo[0], eps); e[1] = upwind_mac(L[1], VR[1], m_lo[1], eps); e[2] = upwind_mac(L[2], VR[2], m_lo[2], eps);
          if (BCP) {
            if (wd & 0xF00F) { FACE_BC(e[0], wd, 0, L[0], VR[0], s0, S_AT(kc, -8L)) FACE_BC(e[1], wd, 12, L[1], VR[1], s0, S_AT(kc, -F.s_row)) }
            if (zw & 15) { FACE_BC(e[2], zw, 0, L[2], VR[2], s0, S_AT(kc - 1, 0L)) }
          }
        }
        if (!UPD) {
          if (own_ij) {
            if (vy && vz) { std_(qex, 0u, e[0]); if (cons) std_(qfx, 0u, e[0] * m_lo[0]); }
            if (vx && vz) { std_(qey, 0u, e[1]); if (cons) std_(qfy, 0u, e[1] * m_lo[1]); }
            if (vx && vy) { std_(qez, 0u, e[2]); if (cons) std_(qfz, 0u, e[2] * m_lo[2]); }
          }
          qex += F.sq[0]; qfx += F.sq[0]; qey += F.sq[1]; qfy += F.sq[1]; qez += F.sq[2]; qfz += F.sq[2];
        } else {
          const double ex = cons ? e[0] * m_lo[0] : e[0], ey = cons ? e[1] * m_lo[1] : e[1], ez = cons ? e[2] * m_lo[2] : e[2];
          if (STEADY || k - 1 >= k0) {                                 // finish plane k-1: its upper y face from the row above, its upper z face = ez
            const double eyu = LP(lE[buf ^ 1]);
            const double ty = cons ? DIVDX(eyu - c_e1, 1) : DIVDX(c_vbar * (eyu - c_e1), 1);
            const double tz = cons ? DIVDX(ez - c_e2, 2) : DIVDX(c_wbar * (ez - c_e2), 2);
            const double ug = c_tx + ty + tz;
            const bool vzp = k - 1 >= F.lo[2] && k - 1 <= F.hi[2];
            if (own_ij && vx && vy && vzp) std_(qn, 0u, c_so - F.dt * ug + F.dt * c_fu);
            qn += F.sqn;
          }
          const double exu = lane_next(ex);                            // the upper x face: the next lane's lower one
          c_tx = cons ? DIVDX(exu - ex, 0) : DIVDX((0.5 * (m_lo[0] + m_up[0])) * (exu - ex), 0);
          c_vbar = 0.5 * (m_lo[1] + m_up[1]); c_wbar = 0.5 * (m_lo[2] + m_up[2]);
          c_e1 = ey; c_e2 = ez; c_so = s0;
          if (fmode == 0) c_fu = P2.f;
          else {
            const long po = (long)(kc - KB) * F.sp[5] + o_f;
            c_fu = ldd(F.pfu[0] + po, 0u) + (F.lapu0 - ldd(F.pfu[1] + po, 0u)) / ldd(F.pfu[2] + po, 0u);
          }
          LS(lE[buf]) = ey;                                     // read by the row below in the next iteration
        }
      }
    }
    si1[0] = si0[0]; si1[1] = si0[1]; si1[2] = si0[2];
    #pragma unroll
    for (int n = 0; n < 6; n++) qp[n] = qc[n];
  };
  #undef CHAIN1
  // The march over ONE plane function in two forms.  Stage C starts at kk = k0, stage D at k0 + 1, the stores at k0 + 2, the update's finishing half
  // at k0 + 3, and loads stop at k1 + 2: all five conditions hold for kk in [k0 + 3, k1 + 1], and there the plane runs with them compiled in (no uniform
  // branches, no PHI copies around them, unconditional loads) -- the steady form; the five planes before and the one or two after test them as before.
  // The steady form carries no boundary code: in a workgroup that runs the boundary body it takes the planes whose three stage planes (kk, kk - 1,
  // kk - 2) stay clear of the z faces when the tile touches no x / y face with a rule (no cell of such a plane is flagged: it is what an unflagged
  // workgroup executes); every other plane of that workgroup runs the tested form with the boundary code.  Same expressions, one barrier per plane in
  // every form; a chunk of at most 3 planes has no steady plane.  Three loops one after the other: the same planes in one loop that chooses the form
  // per plane made every kernel spill (300 to 480 bytes of scratch per lane).
  bool xy_face = false;                                               // the tile comes within one cell of an x / y face that carries a rule (uniform)
  if (BC) {
    const int t0[2] = { r.lo[0] - 1 + BX * ownx, r.lo[1] - 1 + BY * owny }, t1[2] = { t0[0] + G.W - 1, t0[1] + G.ROWS - 1 };
    #pragma unroll
    for (int d = 0; d < 2; d++) xy_face = xy_face || (mode[d][0] && t0[d] <= F.lo[d] + 1) || (mode[d][1] && t1[d] >= F.hi[d] - 1);
  }
  const int kend = k1 + 2 + (UPD ? 1 : 0);
  const int ks0 = BC ? max(k0 + 3, F.lo[2] + 3) : k0 + 3, ks1 = (BC && xy_face) ? ks0 - 1 : (BC ? min(k1 + 1, F.hi[2] - 1) : k1 + 1);
  int kk = k0 - 2;
  for (; kk <= (PEEL ? min(ks0 - 1, kend) : kend); kk++) plane(std::integral_constant<int, PH_EDGE>{}, std::true_type{}, kk);
  if (PEEL) for (; kk <= ks1; kk++) plane(std::integral_constant<int, PH_STEADY>{}, std::false_type{}, kk);
  if (PEEL) for (; kk <= kend; kk++) plane(std::integral_constant<int, PH_EDGE>{}, std::true_type{}, kk);
  #undef F_LOAD
  #undef F_ADVANCE
  #undef S_AT
  #undef BC_V
  #undef FACE_BC
  #undef PREMOD
  #undef Z_WORD
}
// touch = true: the workgroup (bx, by, bz) of tw lanes x th rows, ownx columns its own, comes near a face of F's box that carries a rule for F's component (footprint and rule: godunov_plan.h)
#define MK_TOUCH(touch, F, r, tw, th, ownx, klen, UPD, bx, by, bz) {                                                                    \
    GOD_FOOTPRINT(r.lo, r.hi, tw, th, ownx, klen, UPD, bx, by, bz, a0, a1)                                                                  \
    GOD_TOUCH(touch, a0, a1, F.lo, F.hi, d, bc_mode(F.phys[d][0], F.is_vel != 0, F.c == d), bc_mode(F.phys[d][1], F.is_vel != 0, F.c == d)) }
template <bool BC = true, bool INL = true, bool UPD = false, bool PW2 = false, int SP = SP_RT> __global__ void __launch_bounds__(64 * TNY) kk_mk_F_m(FArgs F, Range3 r, int klen, const double *umax) {
  int bx_, by_, bz_; xcd_remap(bx_, by_, bz_);
  // a workgroup whose tile and k-chunk stay clear of every face that carries a rule runs the body without the boundary code (same values:
  // none of its cells is flagged); compiled into one kernel the lean path keeps its own register allocation (0.69 against 0.96 ms per launch)
  bool touch = false;
  if (BC) MK_TOUCH(touch, F, r, 64, TNY, FNX, klen, UPD, bx_, by_, bz_)
  __shared__ FShared<UPD> S;
  constexpr bool PEEL = SP != SP_RT || !UPD;       // (the update forms with run-time flags stay unpeeled: peeled, the inflow one needs scratch -- profiles/godunov_phases_ab.txt)
  if (BC && touch) mk_F_m_body<BC, INL, UPD, PW2, false, SP, PEEL>(S, F, r, klen, umax, bx_, by_, bz_);
  else mk_F_m_body<false, false, UPD, PW2, false, SP, PEEL>(S, F, r, klen, umax, bx_, by_, bz_);
}
// The remainder column of a one-box level in narrow segments (round 5).  A row of 256 cells is four 62-cell tiles and 8 cells: the fifth tile column
// marched 64 lanes for 8 cells (a fifth of all workgroups at 256^3).  With NCOL that column runs in segments of (cells + 2) lanes, 64 / W rows per wave
// (NAR, see seg_geo): 10 lanes x 6 rows, a workgroup 48 rows of which 46 own cells -- 6 workgroups per k-chunk instead of 43; the other workgroups of the
// column's grid slots leave at once.  ONE launch (as a second launch the 42 workgroups were a round of their own: measured, slower than the full tiles).
// Same body, same values; the update rides along as in the full-width tiles (the shared arrays are addressed flat).
template <bool BC, bool INL, bool UPD, bool PW2, int SP = SP_RT> __global__ void __launch_bounds__(64 * TNY) kk_mk_F_mc(FArgs F, Range3 r, int klen, const double *umax, int full, int segw) {
  int bx_, by_, bz_; xcd_remap(bx_, by_, bz_);
  const bool narrow = bx_ == full;
  Range3 rr = r;
  int tw = 64, th = TNY, ownx = FNX;      // (GOD_COL's map in this kernel's own text, as in kk_vp_F_mc: expanded from the header it changes the code of every instantiation)
  if (narrow) {
    tw = segw; th = TNY * (64 / segw); ownx = segw - 2;
    rr.lo[0] = r.lo[0] + full * FNX;
    if (by_ * (th - 2) > r.hi[1] - r.lo[1]) return;                 // the narrow column needs fewer workgroups along y than the grid has
    bx_ = 0;
  } else rr.hi[0] = r.lo[0] + full * FNX - 1;
  bool touch = false;
  if (BC) MK_TOUCH(touch, F, rr, tw, th, ownx, klen, UPD, bx_, by_, bz_)
  __shared__ FShared<UPD> S;
  constexpr bool PEEL = SP != SP_RT;               // (as in kk_mk_F_m)
  if (narrow) {
    if (BC && touch) mk_F_m_body<BC, INL, UPD, PW2, true, SP, PEEL>(S, F, rr, klen, umax, bx_, by_, bz_, segw);
    else mk_F_m_body<false, false, UPD, PW2, true, SP, PEEL>(S, F, rr, klen, umax, bx_, by_, bz_, segw);
  } else {
    if (BC && touch) mk_F_m_body<BC, INL, UPD, PW2, false, SP, PEEL>(S, F, rr, klen, umax, bx_, by_, bz_);
    else mk_F_m_body<false, false, UPD, PW2, false, SP, PEEL>(S, F, rr, klen, umax, bx_, by_, bz_);
  }
}
// Half workgroups on wide one-box levels.  At 231 to 251 VGPRs a CU holds eight waves of these marches, and in kk_mk_F_mc they are ONE workgroup: one
// batch of loads and one barrier per plane, so all eight wait for memory together and compute together.  Here a workgroup is 64 x THY threads with half
// the shared arrays (32 KB), and two of them share a CU -- the same occupancy, but the two march independently.  Every tile runs the segmented body (NAR)
// in segments of segw = 16 or 32 lanes: THY * 64 / segw rows, all lanes live; grid and chunk rule: god_grid_half.  Same body, same values.
template <bool BC, bool INL, bool UPD, bool PW2, int SP = SP_RT> __global__ void __launch_bounds__(64 * THY, 2) kk_mk_F_mh(FArgs F, Range3 r, int klen, const double *umax, int segw) {
  int bx_, by_, bz_; xcd_remap(bx_, by_, bz_);
  bool touch = false;
  if (BC) MK_TOUCH(touch, F, r, segw, THY * (64 / segw), segw - 2, klen, UPD, bx_, by_, bz_)
  __shared__ FShared<UPD, THY> S;
  constexpr bool PEEL = SP != SP_RT;               // (as in kk_mk_F_m)
  if (BC && touch) mk_F_m_body<BC, INL, UPD, PW2, true, SP, PEEL, THY>(S, F, r, klen, umax, bx_, by_, bz_, segw);
  else mk_F_m_body<false, false, UPD, PW2, true, SP, PEEL, THY>(S, F, r, klen, umax, bx_, by_, bz_, segw);
}
// the launch arguments of the fused march for component c; false when the field layouts do not allow the shared offsets
static bool fused_args(FArgs &F, const GArgs &A, int c, const FV &s, const FV sl[3], const FV &um, const FV &vm, const FV &wm, const FV &force, const FV &macrhs,
                       const FV &sex, const FV &sey, const FV &sez, const FV &flx, const FV &fly, const FV &flz) {
  if (!same_geom(sl[0], sl[1]) || !same_geom(sl[0], sl[2]) || !same_geom(sex, flx) || !same_geom(sey, fly) || !same_geom(sez, flz)) return false;
  const int KB = A.lo[2] - 1;
  const FV *in[9] = { &s, &sl[0], &sl[1], &sl[2], &um, &vm, &wm, &force, &macrhs };
  const int comp[9] = { c, c, c, c, 0, 0, 0, c, 0 }, grp[9] = { 0, 1, 1, 1, 2, 3, 4, 5, 6 };
  for (int f = 0; f < 9; f++) {
    const FV &v = *in[f];
    if (KB < v.a2 || A.hi[2] + 1 + (f == 6 ? 1 : 0) >= v.a2 + v.n2) return false;      // the clamped planes must exist (wm: one face more)
    F.p[f] = (const char *)(v.p + v.sc * comp[f] + (long)v.n0 * v.n1 * (KB - v.a2));
    F.sp[grp[f]] = 8L * v.n0 * v.n1; F.g[grp[f]] = FGeo{ v.a0, v.a1, v.n0 };
  }
  const FV *out[6] = { &sex, &sey, &sez, &flx, &fly, &flz };
  for (int f = 0; f < 6; f++) {
    const FV &v = *out[f];
    F.q[f] = (char *)(v.p + v.sc * c + (long)v.n0 * v.n1 * (KB - v.a2));
    if (f < 3) { F.sq[f] = 8L * v.n0 * v.n1; F.h[f] = FGeo{ v.a0, v.a1, v.n0 }; }
  }
  F.s_row = 8L * s.n0; F.vm_row = 8L * vm.n0;
  const bool cons = A.cons[c] != 0;
  const double dt2 = 0.5 * A.dt, dt3 = A.dt / 3.0, dt4 = A.dt / 4.0, dt6 = A.dt / 6.0;
  F.dt2 = dt2;
  for (int d = 0; d < 3; d++) {
    F.dx[d] = A.dx[d]; F.idx[d] = 1.0 / A.dx[d]; F.tC[d] = (cons ? dt3 : dt6) / A.dx[d]; F.tD[d] = (cons ? dt2 : dt4) / A.dx[d]; F.aD[d] = dt2 / A.dx[d];
    F.lo[d] = A.lo[d]; F.hi[d] = A.hi[d]; F.phys[d][0] = A.phys[d][0]; F.phys[d][1] = A.phys[d][1];
  }
  F.cons = cons ? 1 : 0; F.use_minion = A.use_minion; F.is_vel = A.is_vel; F.c = c;
  F.p2 = (is_pow2(A.dx[0]) && is_pow2(A.dx[1]) && is_pow2(A.dx[2]) && sw().god_p2) ? 1 : 0;
  F.qn = nullptr; F.sqn = 0; F.hn = FGeo{ 0, 0, 0 }; F.pfu[0] = F.pfu[1] = F.pfu[2] = nullptr; F.fmode = 0; F.dt = A.dt; F.lapu0 = 0.0;
  return true;
}
// the update of component c inside the march (UPD): snew, and the forcing term of the update -- the force of this call (fmode 0) or formed in place
// from ext, gp and rho, which must share the layout of `force` (fmode 1)
static bool fused_update_args(FArgs &F, const GArgs &A, int c, const FV &snew, const FV &force, const MkUpdate &U, int ib) {
  const int KB = A.lo[2] - 1;
  if (KB < snew.a2 || A.hi[2] + 1 >= snew.a2 + snew.n2) return false;
  F.qn = (char *)(snew.p + snew.sc * c + (long)snew.n0 * snew.n1 * (KB - snew.a2));
  F.sqn = 8L * snew.n0 * snew.n1; F.hn = FGeo{ snew.a0, snew.a1, snew.n0 };
  F.fmode = U.fmode; F.lapu0 = U.lapu0;
  if (U.fmode == 1) {
    const FV *in[3] = { &U.ext->fabs[ib], &U.gp->fabs[ib], &U.rho->fabs[ib] };
    const int comp[3] = { c, c, 0 };
    for (int f = 0; f < 3; f++) {
      const FV &v = *in[f];
      if (!same_geom(v, force) || v.n2 != force.n2) return false;
      F.pfu[f] = (const char *)(v.p + v.sc * comp[f] + (long)v.n0 * v.n1 * (KB - v.a2));
    }
  }
  return true;
}

// max |umac| over the valid faces of the three MAC components (mkflux.f90:1374-1396)
__global__ void kk_macmax(FV um, FV vm, FV wm, GArgs A, Range3 r, double *out) {
  REDUCE_IJ(r)
  double m = 0.0;
  if (in_ij) REDUCE_KLOOP(r) {
    if (j <= A.hi[1] && k <= A.hi[2]) m = fmax(m, fabs(fv_get(um, i, j, k)));
    if (i <= A.hi[0] && k <= A.hi[2]) m = fmax(m, fabs(fv_get(vm, i, j, k)));
    if (i <= A.hi[0] && j <= A.hi[1]) m = fmax(m, fabs(fv_get(wm, i, j, k)));
  }
  block_atomic_max(out, m);
}
__global__ void kk_velmax(FV u, Range3 r, double *out) {             // velpred.f90:1965-1975
  REDUCE_IJ(r)
  double m = 0.0;
  if (in_ij) REDUCE_KLOOP(r) m = fmax(m, fmax(fmax(fabs(fv_get(u, i, j, k, 0)), fabs(fv_get(u, i, j, k, 1))), fabs(fv_get(u, i, j, k, 2))));
  block_atomic_max(out, m);
}


// ====================================================================================================
// one launch per stage for ALL boxes of a level: a descriptor per box, workgroups bisect a prefix sum for theirs.
// The descriptors are read through the constant address space (scalar loads, never invalidated by the kernel's stores),
// exactly like kernel arguments.
// ====================================================================================================
struct MkD { FV s, sl0, sl1, sl2, um, vm, wm, force, macrhs, sex, sey, sez, flx, fly, flz; GArgs A; Range3 rm, rg, rf; int gs[3], gm[3]; double *umax; };
struct VpD { FV s, sl0, sl1, sl2, force, um, vm, wm;                              GArgs A; Range3 rm, rg, rf; int gs[3], gm[3]; double *umax; };
DEVI int locate_box(const int *start, int nbox, int bid) {
  int lo = 0, hi = nbox - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (as_constant(start + mid) <= bid) lo = mid; else hi = mid - 1; }
  return lo;
}
#define BATCH_LOCATE(D, G)                                                              \
  const int ib_ = locate_box(start, nbox, (int)blockIdx.x);                             \
  const D &q = as_constant(descs + ib_);                                                \
  const int l_ = (int)blockIdx.x - as_constant(start + ib_);                            \
  const int gy_ = q.G[1] > 0 ? q.G[1] : 1;                                               \
  GOD_BATCH_WG(q.G[0], gy_, l_, BX, BY, BZ)
template <class D> __global__ void __launch_bounds__(256) kk_slopes_b(const D *descs, const int *start, int nbox, int dirmask) {
  BATCH_LOCATE(D, gs)
  // gs[1] == 0: the plane flattened over the workgroup's 256 threads (gs[0] workgroups per plane) -- a 14 x 14 plane of a grown 8^3 box is one
  // workgroup at 77 % instead of four 64 x 4 tiles at 19 %
  int i, j, k;
  if (q.gs[1] == 0) {
    const int nx = q.rg.hi[0] - q.rg.lo[0] + 1, l_2 = (int)blockIdx.x - as_constant(start + ib_);
    const int t = (l_2 % q.gs[0]) * 256 + (int)threadIdx.y * 64 + (int)threadIdx.x;
    i = q.rg.lo[0] + t % nx; j = q.rg.lo[1] + t / nx; k = q.rg.lo[2] + l_2 / q.gs[0];
  } else { i = q.rg.lo[0] + BX * 64 + (int)threadIdx.x; j = q.rg.lo[1] + BY * 4 + (int)threadIdx.y; k = q.rg.lo[2] + BZ; }
  if (i > q.rg.hi[0] || j > q.rg.hi[1] || k > q.rg.hi[2]) return;
  slopes_cell(q.s, q.sl0, q.sl1, q.sl2, q.A, dirmask, i, j, k);
}
// per-box maxima (eps of the upwind tests is per box, as in the reference's per-fab calls)
__global__ void kk_macmax_b(const MkD *descs, const int *start, int nbox) {
  BATCH_LOCATE(MkD, gm)
  const int i = q.rf.lo[0] + BX * 64 + (int)threadIdx.x, j = q.rf.lo[1] + BY * 4 + (int)threadIdx.y;
  double m = 0.0;
  if (i <= q.rf.hi[0] && j <= q.rf.hi[1]) for (int k = q.rf.lo[2] + BZ; k <= q.rf.hi[2]; k += q.gm[2]) {
    if (j <= q.A.hi[1] && k <= q.A.hi[2]) m = fmax(m, fabs(fv_get(q.um, i, j, k)));
    if (i <= q.A.hi[0] && k <= q.A.hi[2]) m = fmax(m, fabs(fv_get(q.vm, i, j, k)));
    if (i <= q.A.hi[0] && j <= q.A.hi[1]) m = fmax(m, fabs(fv_get(q.wm, i, j, k)));
  }
  block_atomic_max(q.umax, m);
}
__global__ void kk_velmax_b(const VpD *descs, const int *start, int nbox) {
  BATCH_LOCATE(VpD, gm)
  const int i = q.rm.lo[0] + BX * 64 + (int)threadIdx.x, j = q.rm.lo[1] + BY * 4 + (int)threadIdx.y;
  double m = 0.0;
  if (i <= q.rm.hi[0] && j <= q.rm.hi[1]) for (int k = q.rm.lo[2] + BZ; k <= q.rm.hi[2]; k += q.gm[2])
    m = fmax(m, fmax(fmax(fabs(fv_get(q.s, i, j, k, 0)), fabs(fv_get(q.s, i, j, k, 1))), fabs(fv_get(q.s, i, j, k, 2))));
  block_atomic_max(q.umax, m);
}
// the fused march for every box of a level in one launch (a descriptor per box and component; see kk_batched for the scheme)
struct FBatchD { FArgs F; Range3 r; int klen; const double *umax; int g[3], segw; };      // segw: lanes of a row segment (NAR launches; seg_geo)
template <bool INL, bool PW2 = false, bool NAR = false> __global__ void __launch_bounds__(64 * TNY) kk_mk_F_mb(const FBatchD *descs, const int *start, int nbox) {
  BATCH_LOCATE(FBatchD, g)
  bool touch = false;                                // see kk_mk_F_m
  { const int tw = NAR ? q.segw : 64, th = NAR ? TNY * (64 / q.segw) : TNY; MK_TOUCH(touch, q.F, q.r, tw, th, tw - 2, q.klen, false, BX, BY, BZ) }
  __shared__ FShared<false> S;
  if (touch) mk_F_m_body<true, INL, false, PW2, NAR>(S, q.F, q.r, q.klen, q.umax, BX, BY, BZ, q.segw);
  else mk_F_m_body<false, false, false, PW2, NAR>(S, q.F, q.r, q.klen, q.umax, BX, BY, BZ, q.segw);
}

// host side of a batch: grids of the slope and the reduction launch per box, their prefix sums, and the upload
template <class D> struct GodBatch {
  std::vector<D> d; const D *dev = nullptr; const int *st[2] = { nullptr, nullptr }; int tot[2] = { 0, 0 };
  void finish() {
    const int nb = (int)d.size();
    std::vector<int> start(2 * nb);
    for (int b = 0; b < nb; b++) {
      D &q = d[b];
      const dim3 gs = grid_for(q.rg), gm = reduce_grid(q.rm);
      const dim3 *g[2] = { &gs, &gm }; int *o[2] = { q.gs, q.gm };
      for (int t = 0; t < 2; t++) { o[t][0] = g[t]->x; o[t][1] = g[t]->y; o[t][2] = g[t]->z; start[t * nb + b] = tot[t]; tot[t] += (int)(g[t]->x * g[t]->y * g[t]->z); }
      // the slope launch: the plane flattened over the workgroup when that takes fewer workgroups (kk_slopes_b: gs[1] = 0)
      const int pnx = q.rg.hi[0] - q.rg.lo[0] + 1, pny = q.rg.hi[1] - q.rg.lo[1] + 1;
      if (sw().batch_flat && pnx > 0 && pny > 0 && (pnx * pny + 255) / 256 < (int)(gs.x * gs.y)) {
        const int gfl = (pnx * pny + 255) / 256;
        tot[0] += (gfl - (int)(gs.x * gs.y)) * (int)gs.z;
        q.gs[0] = gfl; q.gs[1] = 0;
      }
    }
    D *dd = (D *)desc_scratch(sizeof(D) * nb); int *ds = (int *)desc_scratch(sizeof(int) * 2 * nb);
    upload_staged(dd, d.data(), sizeof(D) * nb); upload_staged(ds, start.data(), sizeof(int) * 2 * nb);
    dev = dd; for (int t = 0; t < 2; t++) st[t] = ds + t * nb;
  }
};

static void fill_gargs(GArgs &A, const vdn_multifab *s, int ibox, const vdn_bc_tower *bct, int bccomp, int ncomp, const double *dx, double dt) {
  memset(&A, 0, sizeof A);
  BoxP bp = make_boxp(s, ibox, bct);
  for (int d = 0; d < 3; d++) {
    A.lo[d] = bp.lo[d]; A.hi[d] = bp.hi[d]; A.dx[d] = (dx && d < ctx().prm.dm) ? dx[d] : 1.0;      // dx holds dm entries
    for (int sd = 0; sd < 2; sd++) {
      A.phys[d][sd] = bp.phys[d][sd];
      for (int c = 0; c < ncomp && c < 3; c++) A.adv[d][sd][c] = bct->adv_bc(s->lev, ibox + 1, d, sd, bccomp + c);
    }
  }
  A.dt = dt; A.ncomp = ncomp; A.use_minion = ctx().prm.use_minion; A.slope_order = ctx().prm.slope_order; A.outlet2d = ctx().extruded2d ? 1 : 0;
}
static void k2_velpred(const vdn_multifab *u, vdn_multifab **umac, const vdn_multifab *force, const double *dx, double dt, const vdn_bc_tower *bct);
static void k2_mkflux(const vdn_multifab *s, vdn_multifab **sedge, vdn_multifab **flux, vdn_multifab **umac, const vdn_multifab *force,
                      const vdn_multifab *mac_rhs, const double *dx, double dt, const vdn_bc_tower *bct, bool is_vel, int bccomp, const int *is_cons);
// components [c0, c0 + nc) of m: the same boxes and memory, every fab offset by c0 component strides (FV.sc).  A value that owns nothing
// (no destroy): the scalar Godunov kernels take at most three components per launch, so nscal > 3 runs them on windows of three
static vdn_multifab comp_window(const vdn_multifab *m, int c0, int nc) {
  vdn_multifab v = *m;
  v.owns = false; v.nc = nc;
  for (FV &f : v.fabs) f.p += f.sc * c0;
  return v;
}
static FV work_fv(const BoxP &b) {              // a field over the box grown by one, no memory yet
  FV f; f.p = nullptr; f.a0 = b.lo[0] - 1; f.a1 = b.lo[1] - 1; f.a2 = b.lo[2] - 1;
  f.n0 = b.hi[0] - b.lo[0] + 3; f.n1 = b.hi[1] - b.lo[1] + 3; f.n2 = b.hi[2] - b.lo[2] + 3;
  f.sc = (long)f.n0 * f.n1 * f.n2;
  return f;
}
// ---- host side of the fused marches: tiling, grids and forms are godunov_plan.h's -------------------------------------------------------------
// what both predictors set up per box (dm = 3), batched or box by box: the arguments, a work field over the grown box and its bytes, the ranges of the
// slopes (rg: the grown box) and of the faces (rf), the three slope fields -- the step's kept ones (cached: ctx().slope_cache) or ncomp components each
// from the arena -- and whether a face carries a rule (any) or is an inlet (inflow).  is_cons: null for velpred
struct GodBox { GArgs A; FV w, sl[3]; size_t fld; Range3 rg, rf; bool any, inflow; };
static GodBox god_box(const vdn_multifab *s, int ib, const vdn_bc_tower *bct, int bccomp, int ncomp, const double *dx, double dt, bool is_vel, const int *is_cons, bool cached) {
  GodBox B;
  fill_gargs(B.A, s, ib, bct, bccomp, ncomp, dx, dt);
  B.A.is_vel = is_vel ? 1 : 0;
  for (int c = 0; c < ncomp && is_cons; c++) B.A.cons[c] = is_cons[c] ? 1 : 0;
  B.w = work_fv(make_boxp(s, ib, bct)); B.fld = (size_t)B.w.sc * sizeof(double);
  B.any = B.inflow = false;
  for (int d = 0; d < 3; d++) {
    B.rg.lo[d] = B.A.lo[d] - 1; B.rg.hi[d] = B.A.hi[d] + 1; B.rf.lo[d] = B.A.lo[d]; B.rf.hi[d] = B.A.hi[d] + 1;
    B.sl[d] = B.w; B.sl[d].p = cached ? ctx().slope_cache[d][ib] : (double *)arena_alloc(B.fld * ncomp);
    for (int sd = 0; sd < 2; sd++) { B.any = B.any || bc_mode_host(B.A.phys[d][sd]); B.inflow = B.inflow || B.A.phys[d][sd] == VDN_INLET; }
  }
  return B;
}
struct Ext3 { int n[3]; Ext3(const Range3 &r) { for (int d = 0; d < 3; d++) n[d] = r.hi[d] - r.lo[d] + 1; } };
// the grid of a descriptor's box in the batched launch (D: FBatchD, VBatchD)
template <class D> static void batch_grid(D &q) {
  const Ext3 e(q.r);
  const GodGrid G = god_grid_small(e.n[0], e.n[1], e.n[2], sw().god_segw);
  q.klen = G.klen; q.segw = G.segw; for (int d = 0; d < 3; d++) q.g[d] = G.g[d];
}
// the batched march of a level in two launches: the boxes in full-width tiles, then the narrow ones in row segments (seg_geo) -- the descriptors in
// that order, each with the first workgroup of its box in its launch, one upload.  launch: the dispatch of the kernel family
template <class D> static void launch_batched(std::vector<D> &fd, GodForm f, hipStream_t st, void (*launch)(const GodForm &, int, hipStream_t, const D *, const int *, int)) {
  std::stable_partition(fd.begin(), fd.end(), [](const D &q) { return q.segw == 0; });
  const int n = (int)fd.size(), nwide = (int)std::count_if(fd.begin(), fd.end(), [](const D &q) { return q.segw == 0; });
  std::vector<int> start(n);
  int tot[2] = { 0, 0 };
  for (int t = 0; t < n; t++) { int &T = tot[t < nwide ? 0 : 1]; start[t] = T; T += fd[t].g[0] * fd[t].g[1] * fd[t].g[2]; }
  D *dd = (D *)desc_scratch(sizeof(D) * n); int *ds = (int *)desc_scratch(sizeof(int) * n);
  upload_staged(dd, fd.data(), sizeof(D) * n); upload_staged(ds, start.data(), sizeof(int) * n);
  if (nwide) launch(f, tot[0], st, dd, ds, nwide);
  f.nar = true;
  if (nwide < n) launch(f, tot[1], st, dd + nwide, ds + nwide, n - nwide);
}
// one dispatch per kernel family: the instantiation of the form f from the family's list in godunov_plan.h, launched on the grid g and the stream st of
// the dispatching function; a form outside the list is an error.  GOD_X_*: a list entry of a family as such a case, with the family's arguments
#define GOD_CASE(FORM_, K, ...) if (f == FORM_) { hipLaunchKernelGGL(K, g, dim3(64, TNY, 1), 0, st, __VA_ARGS__); return; }
#define GOD_NO_FORM(what) REQUIRE(false, what ": no march of the form bc %d inl %d upd %d pw2 %d sp %d nar %d cols %d", f.bc, f.inl, f.upd, f.pw2, f.sp, f.nar, f.cols)
#define GOD_X_MK_M(bc, inl, upd, pw2, sp, nar, cols) GOD_CASE(GOD_FORM(bc, inl, upd, pw2, sp, nar, cols), (kk_mk_F_m<bc, inl, upd, pw2, sp>), F, r, G.klen, umax)
#define GOD_X_MK_MC(bc, inl, upd, pw2, sp, nar, cols) GOD_CASE(GOD_FORM(bc, inl, upd, pw2, sp, nar, cols), (kk_mk_F_mc<bc, inl, upd, pw2, sp>), F, r, G.klen, umax, G.full, G.segw)
#define GOD_X_MK_MH(bc, inl, upd, pw2, sp, nar, cols) if (f == GOD_FORM_HALF(bc, inl, upd, pw2, sp, nar, cols)) { hipLaunchKernelGGL((kk_mk_F_mh<bc, inl, upd, pw2, sp>), g, dim3(64, THY, 1), 0, st, F, r, G.klen, umax, G.segw); return; }
#define GOD_X_MK_MB(bc, inl, upd, pw2, sp, nar, cols) GOD_CASE(GOD_FORM(bc, inl, upd, pw2, sp, nar, cols), (kk_mk_F_mb<inl, pw2, nar>), dd, ds, n)
// testing build (vdn_last_mkflux_form): the family the last one-box mkflux march came from -- 0: kk_mk_F_m; 1: kk_mk_F_mc; 16 / 32: kk_mk_F_mh in segments of
// that many lanes; -1: none yet
static int g_mk_form = -1;
int mkflux_last_form() { return g_mk_form; }
static void launch_mk(const GodForm &f, const GodGrid &G, hipStream_t st, const FArgs &F, const Range3 &r, const double *umax) {
  const dim3 g(G.g[0], G.g[1], G.g[2]);
  g_mk_form = f.half ? G.segw : f.cols ? 1 : 0;
  GOD_MK_M_FORMS(GOD_X_MK_M) GOD_MK_MC_FORMS(GOD_X_MK_MC) GOD_MK_MH_FORMS(GOD_X_MK_MH) GOD_NO_FORM("mkflux");
}
static void launch_mk_b(const GodForm &f, int tot, hipStream_t st, const FBatchD *dd, const int *ds, int n) {
  const dim3 g(tot);
  GOD_MK_MB_FORMS(GOD_X_MK_MB) GOD_NO_FORM("mkflux, batched");
}

void k_slope(const vdn_multifab *s, vdn_multifab *slope, int dir, int bccomp, const vdn_bc_tower *bct) {
  REQUIRE(s->ng >= 3 && slope->ng == 1 && slope->nc >= s->nc, "k_slope: need s.ng>=3, slope.ng==1, slope.nc>=s.nc");
  if (s->nc > 3) {                                     // windows of three components (comp_window)
    for (int c0 = 0; c0 < s->nc; c0 += 3) {
      const int w = std::min(3, s->nc - c0);
      const vdn_multifab sv = comp_window(s, c0, w);
      vdn_multifab lw = comp_window(slope, c0, w);
      k_slope(&sv, &lw, dir, bccomp + c0, bct);
    }
    return;
  }
  for (int i = 0; i < s->nfabs(); i++) {
    GArgs A; fill_gargs(A, s, i, bct, bccomp, s->nc, nullptr, 0.0);
    Range3 r; for (int d = 0; d < 3; d++) { r.lo[d] = A.lo[d] - 1; r.hi[d] = A.hi[d] + 1; }
    hipLaunchKernelGGL(kk_slopes, grid_for(r), dim3(64, 4, 1), 0, ctx().stream, s->fabs[i], slope->fabs[i], slope->fabs[i], slope->fabs[i], A, r, 1 << dir);
  }
}

// the slope launch of the predictors by itself (unit-test hook): all three directions of the two or three components of s, box by box through launch_slopes,
// so in whichever form the switches and the layouts choose; vmax (may be null): the largest |s| over the valid cells of all boxes rides along, as in velpred
void k_slopes_march(const vdn_multifab *s, vdn_multifab *sl0, vdn_multifab *sl1, vdn_multifab *sl2, int bccomp, const vdn_bc_tower *bct, double *vmax) {
  REQUIRE((s->nc == 2 || s->nc == 3) && s->ng >= 3, "k_slopes_march: s needs 2 or 3 components and 3 ghost cells");
  REQUIRE(sl0->ng == 1 && sl1->ng == 1 && sl2->ng == 1 && sl0->nc == s->nc && sl1->nc == s->nc && sl2->nc == s->nc, "k_slopes_march: the slope multifabs need 1 ghost cell and the components of s");
  hipStream_t st = ctx().stream;
  double *dmax = nullptr;
  if (vmax) { dmax = (double *)arena_alloc(256); HIPCHK(hipMemsetAsync(dmax, 0, sizeof(double), st)); }
  for (int ib = 0; ib < s->nfabs(); ib++) {
    GArgs A; fill_gargs(A, s, ib, bct, bccomp, s->nc, nullptr, 0.0);
    Range3 rg; for (int d = 0; d < 3; d++) { rg.lo[d] = A.lo[d] - 1; rg.hi[d] = A.hi[d] + 1; }
    const FV sl[3] = { sl0->fabs[ib], sl1->fabs[ib], sl2->fabs[ib] };
    launch_slopes(s->fabs[ib], sl, A, rg, s->nc, dmax, st);
  }
  if (vmax) *vmax = read_scalar1(dmax);
}

// one window of at most three components (k_mkflux below); bccomp: the bc-tower component of the window's first component
static bool mkflux_window(const vdn_multifab *s, vdn_multifab **sedge, vdn_multifab **flux, vdn_multifab **umac,
                          const vdn_multifab *force, const vdn_multifab *mac_rhs, const double *dx, double dt,
                          const vdn_bc_tower *bct, bool is_vel, int bccomp, const int *is_cons, const MkUpdate *upd) {
  if (ctx().prm.dm == 2) { k2_mkflux(s, sedge, flux, umac, force, mac_rhs, dx, dt, bct, is_vel, bccomp, is_cons); return false; }
  bool updated = false;
  const int ncomp = s->nc;
  REQUIRE(ncomp <= 3, "mkflux: at most 3 components per window (got %d)", ncomp);
  REQUIRE(s->ng >= 3 && umac[0]->ng >= 1 && force->ng >= 1 && mac_rhs->ng >= 1, "mkflux: ghost widths");
  hipStream_t st = ctx().stream;
  if (use_batched(s) && !sw().godunov_plain) {            // every stage once for all boxes of the level: the slopes, then stages B + C + D in one march (mk_F_m_body)
    size_t mark = arena_mark();
    const int nb = s->nfabs();
    GodBatch<MkD> B; B.d.resize(nb);
    double *umax = (double *)arena_alloc(sizeof(double) * nb);
    HIPCHK(hipMemsetAsync(umax, 0, sizeof(double) * nb, st));
    std::vector<FBatchD> fd((size_t)nb * ncomp);
    bool ok = true, inflow = false;
    for (int ib = 0; ib < nb && ok; ib++) {
      MkD &q = B.d[ib];
      const GodBox X = god_box(s, ib, bct, bccomp, ncomp, dx, dt, is_vel, is_cons, false);
      q.A = X.A; q.sl0 = X.sl[0]; q.sl1 = X.sl[1]; q.sl2 = X.sl[2]; q.rg = X.rg; q.rf = q.rm = X.rf;
      q.s = s->fabs[ib]; q.um = umac[0]->fabs[ib]; q.vm = umac[1]->fabs[ib]; q.wm = umac[2]->fabs[ib]; q.force = force->fabs[ib]; q.macrhs = mac_rhs->fabs[ib];
      q.sex = sedge[0]->fabs[ib]; q.sey = sedge[1]->fabs[ib]; q.sez = sedge[2]->fabs[ib]; q.flx = flux[0]->fabs[ib]; q.fly = flux[1]->fabs[ib]; q.flz = flux[2]->fabs[ib];
      q.umax = umax + ib;
      inflow = inflow || X.inflow;
      for (int c0 = 0; c0 < ncomp && ok; c0++) {
        FBatchD &f = fd[(size_t)c0 * nb + ib];
        ok = fused_args(f.F, q.A, c0, q.s, X.sl, q.um, q.vm, q.wm, q.force, q.macrhs, q.sex, q.sey, q.sez, q.flx, q.fly, q.flz);
        f.r = q.rf; f.umax = q.umax;
        batch_grid(f);
      }
    }
    if (ok) {
      B.finish();
      hipLaunchKernelGGL(kk_macmax_b, dim3(B.tot[1]), dim3(64, 4, 1), 0, st, B.dev, B.st[1], nb);      // per-box max |umac|
      hipLaunchKernelGGL(kk_slopes_b<MkD>, dim3(B.tot[0]), dim3(64, 4, 1), 0, st, B.dev, B.st[0], nb, 7);
      launch_batched(fd, god_mk_form(true, inflow, fd[0].F.p2 != 0, false, SP_RT, false, true), st, launch_mk_b);      // (batched: inflow and p2 alone decide)
      arena_release(mark);
      return false;
    }
    arena_release(mark);                               // a box's layouts refused: the level runs box by box
  }
  for (int ib = 0; ib < s->nfabs(); ib++) {
    size_t mark = arena_mark();
    const bool cached = is_vel && ncomp == 3 && (int)ctx().slope_src.size() == s->nfabs() && ctx().slope_src[ib] == s->fabs[ib].p;      // advance_timestep: velpred's slopes of the same u
    const GodBox X = god_box(s, ib, bct, bccomp, ncomp, dx, dt, is_vel, is_cons, cached);
    const GArgs &A = X.A; const FV *sl = X.sl; const Range3 &rg = X.rg, &rf = X.rf;
    const FV &um = umac[0]->fabs[ib], &vm = umac[1]->fabs[ib], &wm = umac[2]->fabs[ib];
    const bool mm_keep = (int)ctx().macmax_cache.size() == s->nfabs();       // advance_timestep: one reduction serves both mkflux calls of the step
    double *umax = mm_keep ? ctx().macmax_cache[ib] : (double *)arena_alloc(256);
    if (!(mm_keep && ctx().macmax_src[ib] == um.p)) {
      HIPCHK(hipMemsetAsync(umax, 0, sizeof(double), st));
      hipLaunchKernelGGL(kk_macmax, reduce_grid(rf), dim3(64, 4, 1), 0, st, um, vm, wm, A, rf, umax);
      if (mm_keep) ctx().macmax_src[ib] = um.p;
    }
    if (!cached) launch_slopes(s->fabs[ib], sl, A, rg, ncomp, nullptr, st);
    FArgs FA[3];
    bool fused = !sw().godunov_plain;
    for (int c0 = 0; c0 < ncomp && fused; c0++)
      fused = fused_args(FA[c0], A, c0, s->fabs[ib], sl, um, vm, wm, force->fabs[ib], mac_rhs->fabs[ib], sedge[0]->fabs[ib], sedge[1]->fabs[ib], sedge[2]->fabs[ib],
                         flux[0]->fabs[ib], flux[1]->fabs[ib], flux[2]->fabs[ib]);
    if (fused) {                   // stages B + C + D in one march per component, boundary rules inside (see mk_F_m_body)
      bool do_upd = upd && sw().god_update;                  // (every box of a box-by-box level: the conditions are geometric and the same for all of them -- checked below)
      for (int c0 = 0; c0 < ncomp && do_upd; c0++) do_upd = fused_update_args(FA[c0], A, c0, upd->snew->fabs[ib], force->fabs[ib], *upd, ib);
      // full 62-cell tiles, or where the form allows it and it saves workgroups the remainder column in narrow segments (kk_mk_F_mc)
      const Ext3 e(rf);
      const GodGrid gF = god_grid_tiles(e.n[0], e.n[1], e.n[2], sw().fused_kchunks);
      GodGrid gM = gF;
      const bool cols = god_grid_cols(e.n[0], e.n[1], e.n[2], sw().god_narrow, gM);
      // a wide box: half workgroups in place of the column grid (kk_mk_F_mh)
      const GodHalf H = god_half_switch(sw().god_narrow);
      const bool half = god_half_fits(e.n[0], e.n[1], H.on, H.min);
      const GodGrid gH = half ? god_grid_half(e.n[0], e.n[1], e.n[2], H.W, sw().fused_kchunks) : gF;
      for (int c0 = 0; c0 < ncomp; c0++) {
        const GodForm f = god_mk_form(X.any, X.inflow, FA[c0].p2 != 0, do_upd, god_mk_sp(FA[c0].cons != 0, FA[c0].use_minion != 0, FA[c0].fmode), cols, false, half);
        launch_mk(f, f.half ? gH : f.cols ? gM : gF, st, FA[c0], rf, umax);
      }
      REQUIRE(ib == 0 || updated == do_upd, "mkflux: the update would ride along on some boxes of the level only");
      updated = do_upd;
    } else {                       // the face-centred stages: VDN_GODUNOV_PLAIN, or field layouts the fused march refuses
      REQUIRE(!updated, "mkflux: the update rode along on an earlier box of the level but cannot on box %d", ib);      // (every box or none)
      FV SI = X.w, SC = X.w;
      SI.p = (double *)arena_alloc(X.fld * 3 * ncomp);
      SC.p = (double *)arena_alloc(X.fld * 6 * ncomp);
      hipLaunchKernelGGL(kk_mk_B, grid_for(rg), dim3(64, 4, 1), 0, st, s->fabs[ib], sl[0], sl[1], sl[2], um, vm, wm, force->fabs[ib], mac_rhs->fabs[ib], SI, A, rg, umax);
      hipLaunchKernelGGL(kk_mk_C, grid_for(rg), dim3(64, 4, 1), 0, st, s->fabs[ib], sl[0], sl[1], sl[2], um, vm, wm, force->fabs[ib], mac_rhs->fabs[ib], SI, SC, A, rg, umax);
      hipLaunchKernelGGL(kk_mk_D, grid_for(rf), dim3(64, 4, 1), 0, st, s->fabs[ib], sl[0], sl[1], sl[2], um, vm, wm, force->fabs[ib], mac_rhs->fabs[ib], SC,
                         sedge[0]->fabs[ib], sedge[1]->fabs[ib], sedge[2]->fabs[ib], flux[0]->fabs[ib], flux[1]->fabs[ib], flux[2]->fabs[ib], A, rf, umax);
    }
    arena_release(mark);
  }
  return updated;
}

// upd: the caller would run update_3d on the result next (one level): where the fused march is taken -- a level of one box -- the update of
// every component runs inside it, sedge / flux stay unwritten and the call returns true; otherwise false and the caller updates as usual.
// More than three components (the scalars of nscal > 3) run as windows of three: offset views of s, force, sedge, flux and snew, the bc
// components bccomp + c0 and the conservative flags from is_cons + c0.  Every window sees the same umac and so the same per-box dead band
// (kk_macmax: the same maximum; kept once per step in macmax_cache on a level of one box), and nscal <= 3 is the one call it always was.
bool k_mkflux(const vdn_multifab *s, vdn_multifab **sedge, vdn_multifab **flux, vdn_multifab **umac,
              const vdn_multifab *force, const vdn_multifab *mac_rhs, const double *dx, double dt,
              const vdn_bc_tower *bct, bool is_vel, const int *is_cons, const MkUpdate *upd) {
  Prof prof_("mkflux");
  const int ncomp = s->nc, dm = ctx().prm.dm;
  const int bccomp = is_vel ? 0 : bct->dm;            // mkflux.f90:62-66
  if (ncomp <= 3) return mkflux_window(s, sedge, flux, umac, force, mac_rhs, dx, dt, bct, is_vel, bccomp, is_cons, upd);
  REQUIRE(!is_vel && ncomp <= VDN_MAXCOMP, "mkflux: %d components (velocity: dm; scalars: at most %d)", ncomp, VDN_MAXCOMP);
  REQUIRE(force->nc >= ncomp && (!upd || (upd->fmode == 0 && upd->snew->nc >= ncomp)), "mkflux: force / snew need the components of s");
  for (int d = 0; d < dm; d++) REQUIRE(sedge[d]->nc >= ncomp && flux[d]->nc >= ncomp, "mkflux: sedge / flux need the components of s");
  bool updated = false;
  for (int c0 = 0; c0 < ncomp; c0 += 3) {
    const int w = std::min(3, ncomp - c0);
    const vdn_multifab sv = comp_window(s, c0, w), fw = comp_window(force, c0, w);
    vdn_multifab ew[3], xw[3], nw;
    vdn_multifab *ep[3] = { nullptr, nullptr, nullptr }, *xp[3] = { nullptr, nullptr, nullptr };
    for (int d = 0; d < dm; d++) { ew[d] = comp_window(sedge[d], c0, w); xw[d] = comp_window(flux[d], c0, w); ep[d] = &ew[d]; xp[d] = &xw[d]; }
    MkUpdate U;
    if (upd) { U = *upd; nw = comp_window(upd->snew, c0, w); U.snew = &nw; }
    const bool u = mkflux_window(&sv, ep, xp, umac, &fw, mac_rhs, dx, dt, bct, is_vel, bccomp + c0, is_cons + c0, upd ? &U : nullptr);
    REQUIRE(c0 == 0 || u == updated, "mkflux: the update rode along in some component windows of the level only");    // every window or none
    updated = u;
  }
  return updated;
}

// ====================================================================================================
// velpred
// ====================================================================================================
// predictor pair of ALL three velocity components on the lower D-face of cell (i,j,k), after bc
// (velpred.f90:2019-2079 x, 2105-2165 y, 2283-2343 z)
template <int D> DEVI void vp_pair(const GArgs &A, const FV &u, const FV &slp, const FV &force, int i, int j, int k, double L[3], double R[3]) {
  const double dt2 = 0.5 * A.dt;
  const double ul = ld<D>(u, i, j, k, -1, D), ur = fv_get(u, i, j, k, D);
  double cfl_l;
  if (D == 1) cfl_l = dt2 * fmax(0.0, ul / A.dx[1]);       // velpred.f90:2108: division inside max()
  else cfl_l = dt2 * fmax(0.0, ul) / A.dx[D];
  const double cfl_r = dt2 * fmin(0.0, ur) / A.dx[D];
  #pragma unroll
  for (int c = 0; c < 3; c++) {
    L[c] = ld<D>(u, i, j, k, -1, c) + (0.5 - cfl_l) * ld<D>(slp, i, j, k, -1, c);
    R[c] = fv_get(u, i, j, k, c) - (0.5 + cfl_r) * fv_get(slp, i, j, k, c);
    if (A.use_minion) { L[c] = L[c] + dt2 * ld<D>(force, i, j, k, -1, c); R[c] = R[c] + dt2 * fv_get(force, i, j, k, c); }
  }
  const int side = face_side<D>(A, i, j, k);
  if (side >= 0) {
    #pragma unroll
    for (int c = 0; c < 3; c++) {
      const double ghost = (side == 0) ? ld<D>(u, i, j, k, -1, c) : fv_get(u, i, j, k, c);
      bc_pair(L[c], R[c], A.phys[D][side], side, true, c == D, ghost, D == 0 && side == 1 && !A.outlet2d);   // :2075 quirk
    }
  }
}

// stage B: UI[(D*3 + c)] = uimh_D component c  (velpred.f90:2081-2098 etc.)
template <int D> DEVI void vp_B_one(const GArgs &A, const FV &u, const FV &slp, const FV &force, const FV &UI, int i, int j, int k, double eps) {
  if (coord<D>(i, j, k) < A.lo[D]) return;
  double L[3], R[3];
  vp_pair<D>(A, u, slp, force, i, j, k, L, R);
  const double uavg = 0.5 * (L[D] + R[D]);
  const bool test = ((L[D] <= 0.0 && R[D] >= 0.0) || (fabs(L[D] + R[D]) < eps));
  double un = (uavg > 0.0) ? L[D] : R[D];
  un = test ? 0.0 : un;
  #pragma unroll
  for (int c = 0; c < 3; c++) {
    double out;
    if (c == D) out = un;
    else {
      double v = (un > 0.0) ? L[c] : R[c];
      double av = 0.5 * (L[c] + R[c]);
      out = (fabs(un) < eps) ? av : v;
    }
    fv_at(UI, i, j, k, D * 3 + c) = out;
  }
}
DEVI void vp_B_cell(const FV &u, const FV &sl0, const FV &sl1, const FV &sl2, const FV &force, const FV &UI, const GArgs &A, int i, int j, int k, double eps) {
  vp_B_one<0>(A, u, sl0, force, UI, i, j, k, eps);
  vp_B_one<1>(A, u, sl1, force, UI, i, j, k, eps);
  vp_B_one<2>(A, u, sl2, force, UI, i, j, k, eps);
}
__global__ void __launch_bounds__(256) kk_vp_B(FV u, FV sl0, FV sl1, FV sl2, FV force, FV UI, GArgs A, Range3 r, const double *umax) {
  THREAD_IJK(r)
  if (!in_range) return;
  vp_B_cell(u, sl0, sl1, sl2, force, UI, A, i, j, k, eps_from(umax));
}

// stage C: component C on D-faces corrected by the third direction O = 3-C-D
// (uimhyz = (C=0,D=1) velpred.f90:2466-2503, wimhxy = (C=2,D=0) 2189-2229, ...)
// XC component index: C*2 + (D > C ? D-1 : D)
DEVI int xc_idx(int C, int D) { return C * 2 + (D > C ? D - 1 : D); }
template <int C, int D> DEVI void vp_C_one(const GArgs &A, const FV &u, const FV &slp, const FV &force, const FV &UI, const FV &XC,
                                           int i, int j, int k, double eps) {
  constexpr int O = 3 - C - D;
  const int qd = coord<D>(i, j, k), qo = coord<O>(i, j, k);
  if (qd < A.lo[D] || qo < A.lo[O] || qo > A.hi[O]) return;
  double Lv[3], Rv[3];
  vp_pair<D>(A, u, slp, force, i, j, k, Lv, Rv);
  const double dt6 = A.dt / 6.0;
  const int ci = i - (D == 0), cj = j - (D == 1), ck = k - (D == 2);
  double L = Lv[C] - (dt6 / A.dx[O]) * (ld<O>(UI, ci, cj, ck, 1, O * 3 + O) + fv_get(UI, ci, cj, ck, O * 3 + O))
                                     * (ld<O>(UI, ci, cj, ck, 1, O * 3 + C) - fv_get(UI, ci, cj, ck, O * 3 + C));
  double R = Rv[C] - (dt6 / A.dx[O]) * (ld<O>(UI, i, j, k, 1, O * 3 + O) + fv_get(UI, i, j, k, O * 3 + O))
                                     * (ld<O>(UI, i, j, k, 1, O * 3 + C) - fv_get(UI, i, j, k, O * 3 + C));
  const int side = face_side<D>(A, i, j, k);
  if (side >= 0) bc_pair(L, R, A.phys[D][side], side, true, false, side == 0 ? ld<D>(u, i, j, k, -1, C) : fv_get(u, i, j, k, C), false);
  const double un = fv_get(UI, i, j, k, D * 3 + D);
  const double v = (un > 0.0) ? L : R;
  const double av = 0.5 * (L + R);
  fv_at(XC, i, j, k, xc_idx(C, D)) = (fabs(un) < eps) ? av : v;
}
DEVI void vp_C_cell(const FV &u, const FV &sl0, const FV &sl1, const FV &sl2, const FV &force, const FV &UI, const FV &XC, const GArgs &A, int i, int j, int k, double eps) {
  vp_C_one<0, 1>(A, u, sl1, force, UI, XC, i, j, k, eps);
  vp_C_one<0, 2>(A, u, sl2, force, UI, XC, i, j, k, eps);
  vp_C_one<1, 0>(A, u, sl0, force, UI, XC, i, j, k, eps);
  vp_C_one<1, 2>(A, u, sl2, force, UI, XC, i, j, k, eps);
  vp_C_one<2, 0>(A, u, sl0, force, UI, XC, i, j, k, eps);
  vp_C_one<2, 1>(A, u, sl1, force, UI, XC, i, j, k, eps);
}
__global__ void __launch_bounds__(256) kk_vp_C(FV u, FV sl0, FV sl1, FV sl2, FV force, FV UI, FV XC, GArgs A, Range3 r, const double *umax) {
  THREAD_IJK(r)
  if (!in_range) return;
  vp_C_cell(u, sl0, sl1, sl2, force, UI, XC, A, i, j, k, eps_from(umax));
}

// stage D: the MAC velocity on valid D-faces (velpred.f90:2616-2660, 2666-2710, 2372-2416)
template <int D> DEVI void vp_D_one(const GArgs &A, const FV &u, const FV &slp, const FV &force, const FV &UI, const FV &XC, const FV &umac,
                                    int i, int j, int k, double eps) {
  constexpr int T1 = (D == 0) ? 1 : 0, T2 = (D == 2) ? 1 : 2;
  if (coord<T1>(i, j, k) > A.hi[T1] || coord<T2>(i, j, k) > A.hi[T2]) return;
  double Lv[3], Rv[3];
  vp_pair<D>(A, u, slp, force, i, j, k, Lv, Rv);
  const double dt2 = 0.5 * A.dt, dt4 = A.dt / 4.0;
  double LR[2] = { Lv[D], Rv[D] };
  #pragma unroll
  for (int sd = 0; sd < 2; sd++) {
    const int ci = i - ((sd == 0) && D == 0), cj = j - ((sd == 0) && D == 1), ck = k - ((sd == 0) && D == 2);
    double v = LR[sd]
      - (dt4 / A.dx[T1]) * (ld<T1>(UI, ci, cj, ck, 1, T1 * 3 + T1) + fv_get(UI, ci, cj, ck, T1 * 3 + T1))
                         * (ld<T1>(XC, ci, cj, ck, 1, xc_idx(D, T1)) - fv_get(XC, ci, cj, ck, xc_idx(D, T1)))
      - (dt4 / A.dx[T2]) * (ld<T2>(UI, ci, cj, ck, 1, T2 * 3 + T2) + fv_get(UI, ci, cj, ck, T2 * 3 + T2))
                         * (ld<T2>(XC, ci, cj, ck, 1, xc_idx(D, T2)) - fv_get(XC, ci, cj, ck, xc_idx(D, T2)));
    if (!A.use_minion) v = v + dt2 * fv_get(force, ci, cj, ck, D);
    LR[sd] = v;
  }
  const double L = LR[0], R = LR[1];
  const double uavg = 0.5 * (L + R);
  const bool test = ((L <= 0.0 && R >= 0.0) || (fabs(L + R) < eps));
  double v = (uavg > 0.0) ? L : R;
  v = test ? 0.0 : v;
  const int side = face_side<D>(A, i, j, k);
  if (side >= 0) {                                   // velpred.f90:2642-2659
    const int ph = A.phys[D][side];
    if (ph == VDN_SLIP_WALL || ph == VDN_NO_SLIP_WALL) v = 0.0;
    else if (ph == VDN_INLET) v = (side == 0) ? ld<D>(u, i, j, k, -1, D) : fv_get(u, i, j, k, D);
    else if (ph == VDN_OUTLET) v = (side == 0) ? fmin(R, 0.0) : fmax(L, 0.0);
  }
  fv_at(umac, i, j, k) = v;
}
DEVI void vp_D_cell(const FV &u, const FV &sl0, const FV &sl1, const FV &sl2, const FV &force, const FV &UI, const FV &XC, const FV &um, const FV &vm, const FV &wm,
                    const GArgs &A, int i, int j, int k, double eps) {
  vp_D_one<0>(A, u, sl0, force, UI, XC, um, i, j, k, eps);
  vp_D_one<1>(A, u, sl1, force, UI, XC, vm, i, j, k, eps);
  vp_D_one<2>(A, u, sl2, force, UI, XC, wm, i, j, k, eps);
}
__global__ void __launch_bounds__(256) kk_vp_D(FV u, FV sl0, FV sl1, FV sl2, FV force, FV UI, FV XC, FV um, FV vm, FV wm, GArgs A, Range3 r, const double *umax) {
  THREAD_IJK(r)
  if (!in_range) return;
  vp_D_cell(u, sl0, sl1, sl2, force, UI, XC, um, vm, wm, A, i, j, k, eps_from(umax));
}

// the upwinded state of stage C (vp_C_one) from the normal velocity un
DEVI double vp_up(double un, double L, double R, double eps) {
  const double v = (un > 0.0) ? L : R;
  const double av = 0.5 * (L + R);
  return (fabs(un) < eps) ? av : v;
}

// ---- velpred: stages B + C + D in one march (all three components; the scheme of mk_F_m_body) --------------------------------------------
// Iteration kk loads plane kk (u, nine slopes, force) and runs stage B on plane kk (UI: the nine upwinded states on the cell's lower faces),
// stage C on plane kk-1 (XC: six transverse-corrected states) and stage D on plane kk-2 (the MAC velocity on the lower faces).  UI and XC
// stay in registers; upper-face values come from the next lane (DPP), the next row (LDS, written one iteration earlier) and, along z, from the
// stage that ran earlier in the same iteration.  A cell carries its eighteen bases from stage B to stage C and the three normal ones on to
// stage D (the face-centred stages recompute them: six f64 divisions per cell and stage).  Every expression is the one of vp_B_one /
// vp_C_one / vp_D_one in the same order (tests/test_kernels_gpu.py::test_velpred, test_godunov_marching_equals_face_centred).
// Boundary rules as packed per-thread codes (mk_F_m_body): bc_pair leaves L = R = v, v one of {ghost, 0, inner, clamped inner}; the
// hi-x OUTLET quirk of velpred.f90:2075 (min instead of max on the normal component) is the code 4 in place of 5 in stages B / premod.
struct VArgs {
  const char *pu, *psl[3], *pf;       // component 0 of u, the three slope fabs and the force at plane KB
  long sc_u, sc_sl, sc_f;             // bytes between components
  long sp_u, sp_sl, sp_f; FGeo g_u, g_sl, g_f;
  char *q[3]; long sq[3]; FGeo h[3];  // umac, vmac, wmac
  long u_row;
  double dt2, dx[3], tC[3], tD[3];    // tC[O] = (dt/6) / dx[O],  tD[T] = (dt/4) / dx[T]
  double idx[3]; int p2;              // as in FArgs: 1 / dx, every dx a power of two (P2 kernels multiply)
  int lo[3], hi[3], phys[3][2], use_minion, outlet2d;
};
DEVI int vp_code_B(int phys, int D, int side, int c, int outlet2d) {
  if (phys == VDN_INLET) return 1;
  if (phys == VDN_SLIP_WALL) return c == D ? 2 : 3;
  if (phys == VDN_NO_SLIP_WALL) return 2;
  if (phys == VDN_OUTLET) return c == D ? ((side == 0 || (D == 0 && !outlet2d)) ? 4 : 5) : 3;
  return 0;
}
DEVI int vp_code_D(int phys, int side) {
  if (phys == VDN_SLIP_WALL || phys == VDN_NO_SLIP_WALL) return 2;
  if (phys == VDN_INLET) return 1;
  if (phys == VDN_OUTLET) return side ? 5 : 4;
  return 0;
}
template <int D> DEVI void vpf_emit(double ui[3], const double L[3], const double R[3], double eps) {      // vp_B_one's upwinding into registers
  const double uavg = 0.5 * (L[D] + R[D]);
  const bool test = ((L[D] <= 0.0 && R[D] >= 0.0) || (fabs(L[D] + R[D]) < eps));
  double un = (uavg > 0.0) ? L[D] : R[D];
  un = test ? 0.0 : un;
  #pragma unroll
  for (int c = 0; c < 3; c++) {
    if (c == D) ui[c] = un;
    else {
      const double v = (un > 0.0) ? L[c] : R[c];
      const double av = 0.5 * (L[c] + R[c]);
      ui[c] = (fabs(un) < eps) ? av : v;
    }
  }
}
DEVI double vpf_riemann(double L, double R, double eps) {            // the state of vp_D_one before its boundary rule
  const double uavg = 0.5 * (L + R);
  const bool test = ((L <= 0.0 && R >= 0.0) || (fabs(L + R) < eps));
  const double v = (uavg > 0.0) ? L : R;
  return test ? 0.0 : v;
}
template <bool BC, bool INL, bool PW2, bool NAR = false, int SP = SP_RT> __device__ __forceinline__ void vp_F_m_body(const VArgs &F, const Range3 &r, int klen, const double *umax, const int BX, const int BY, const int BZ, const int segw = 64) {
  __shared__ double lB[3][TNY][64], lUI[3][TNY][64], lC[2][TNY][64], lXC[2][TNY][64], lD[TNY][64];
  const SegGeo G = seg_geo<NAR>(segw);
  const int lane = G.lane, row = G.row;
  const int ownx = NAR ? G.W - 2 : FNX, owny = NAR ? G.ROWS - 2 : FNY;
  GOD_CELL(r.lo, r.hi, ownx, owny, BX, BY, lane, row, G.live, i, j, own_ij)      // the tile -> cell map: godunov_plan.h
  const int ic = min(max(i, F.lo[0] - 1), F.hi[0] + 1), jc = min(max(j, F.lo[1] - 1), F.hi[1] + 1);
  const bool ing_ij = i == ic && j == jc;
  const bool vx = i >= F.lo[0] && i <= F.hi[0], vy = j >= F.lo[1] && j <= F.hi[1];
  const int rowm = G.rowm, rowp = G.rowp;
  GOD_PLANES(r.lo[2], r.hi[2], klen, BZ, k0, k1)
  const int KB = F.lo[2] - 1, KT = F.hi[2] + 1;
  const double eps = eps_from(umax);
  // packed boundary codes of this thread: wf: x-face (3 comps x 4 bits, +8 = hi side), y-face (bits 12..23), stage-D code of the x-face (24..27) and
  // of the y-face (28..31);  wpx / wpy: rule on the bases of the lowest valid cell (3 x 4 bits) and of the highest (bits 12..23)
  unsigned wf = 0, wpx = 0, wpy = 0;
  if (BC) {
    #pragma unroll
    for (int c = 0; c < 3; c++) {
      if (ing_ij && i == F.lo[0]) wf |= (unsigned)vp_code_B(F.phys[0][0], 0, 0, c, F.outlet2d) << (4 * c);
      if (ing_ij && i == F.hi[0] + 1) { const int cd = vp_code_B(F.phys[0][1], 0, 1, c, F.outlet2d); if (cd) wf |= (unsigned)(cd | 8) << (4 * c); }
      if (ing_ij && j == F.lo[1]) wf |= (unsigned)vp_code_B(F.phys[1][0], 1, 0, c, F.outlet2d) << (12 + 4 * c);
      if (ing_ij && j == F.hi[1] + 1) { const int cd = vp_code_B(F.phys[1][1], 1, 1, c, F.outlet2d); if (cd) wf |= (unsigned)(cd | 8) << (12 + 4 * c); }
      if (ic == F.lo[0]) wpx |= (unsigned)vp_code_B(F.phys[0][0], 0, 0, c, F.outlet2d) << (4 * c);
      if (ic == F.hi[0]) wpx |= (unsigned)vp_code_B(F.phys[0][1], 0, 1, c, F.outlet2d) << (12 + 4 * c);
      if (jc == F.lo[1]) wpy |= (unsigned)vp_code_B(F.phys[1][0], 1, 0, c, F.outlet2d) << (4 * c);
      if (jc == F.hi[1]) wpy |= (unsigned)vp_code_B(F.phys[1][1], 1, 1, c, F.outlet2d) << (12 + 4 * c);
    }
    if (ing_ij && i == F.lo[0]) wf |= (unsigned)vp_code_D(F.phys[0][0], 0) << 24;
    if (ing_ij && i == F.hi[0] + 1) { const int cd = vp_code_D(F.phys[0][1], 1); if (cd) wf |= (unsigned)(cd | 8) << 24; }
    if (ing_ij && j == F.lo[1]) wf |= (unsigned)vp_code_D(F.phys[1][0], 0) << 28;
    if (ing_ij && j == F.hi[1] + 1) { const int cd = vp_code_D(F.phys[1][1], 1); if (cd) wf |= (unsigned)(cd | 8) << 28; }
  }
  // per-thread plane pointers (the thread's column): inputs at the plane the next loads take (kcur), outputs at the plane stage D emits next
  int kcur = min(max(k0 - 2, KB), KT);
  const char *pu = F.pu + (long)(kcur - KB) * F.sp_u + fg_off(F.g_u, ic, jc);
  const char *ps0 = F.psl[0] + (long)(kcur - KB) * F.sp_sl + fg_off(F.g_sl, ic, jc), *ps1 = F.psl[1] + (long)(kcur - KB) * F.sp_sl + fg_off(F.g_sl, ic, jc), *ps2 = F.psl[2] + (long)(kcur - KB) * F.sp_sl + fg_off(F.g_sl, ic, jc);
  const char *pf = F.pf + (long)(kcur - KB) * F.sp_f + fg_off(F.g_f, ic, jc);
  char *qu = F.q[0] + (long)(k0 - KB) * F.sq[0] + fg_off(F.h[0], i, j), *qv = F.q[1] + (long)(k0 - KB) * F.sq[1] + fg_off(F.h[1], i, j), *qw = F.q[2] + (long)(k0 - KB) * F.sq[2] + fg_off(F.h[2], i, j);
  // state carried from plane to plane
  double Lb1[3][3], Rb1[3][3], ui1[3][3];          // plane kk-1: bases [D][c], UI [D][c] on the lower faces
  double LbD[3], RbD[3], sm2[3], xc2[6];           // plane kk-2: normal bases, UI[T][T](+) + UI[T][T], XC on the lower faces
  #pragma unroll
  for (int d = 0; d < 3; d++) { LbD[d] = 0.0; RbD[d] = 0.0; sm2[d] = 0.0; for (int c = 0; c < 3; c++) { Lb1[d][c] = 0.0; Rb1[d][c] = 0.0; ui1[d][c] = 0.0; } }
  #pragma unroll
  for (int n = 0; n < 6; n++) xc2[n] = 0.0;
  double LzB[3] = { 0.0, 0.0, 0.0 }, LzC[2] = { 0.0, 0.0 }, LzD = 0.0;
  #define U_AT(kpl, dbytes, c) (INL ? ldd(pu + (long)((kpl) - kcur) * F.sp_u + (dbytes) + (long)(c) * F.sc_u, 0u) : 0.0)
  #define BC_V(v, code, in, ghost_expr) { const int cd_ = (code); const double in_ = (in); double v_ = in_;                      \
      if (cd_ == 4) v_ = fmin(in_, 0.0); if (cd_ == 5) v_ = fmax(in_, 0.0); if (cd_ == 2) v_ = 0.0; if (cd_ == 1) v_ = (ghost_expr); v = v_; }
  // the face rule on a pair (4-bit field f4: code, +8 = hi face): both states become v
  #define PAIR_BC(L, Rr, f4, own_expr, ghost_expr) { const int f_ = (int)(f4) & 15;                                              \
      if (f_) { const bool hi_ = (f_ & 8) != 0; double o_; BC_V(o_, f_ & 7, hi_ ? (L) : (Rr), hi_ ? (own_expr) : (ghost_expr)) L = o_; Rr = o_; } }
  #define OUT_BC(out, f4, L, Rr, own_expr, ghost_expr) { const int f_ = (int)(f4) & 15;                                          \
      if (f_) { const bool hi_ = (f_ & 8) != 0; double o_; BC_V(o_, f_ & 7, hi_ ? (L) : (Rr), hi_ ? (own_expr) : (ghost_expr)) out = o_; } }
  #define PREMOD(Lb_, Rb_, a4, b4, gl_expr, gh_expr) { const int a_ = (int)(a4) & 7; if (a_) { double o_; BC_V(o_, a_, Rb_, gl_expr) Rb_ = o_; }  \
                                                       const int b_ = (int)(b4) & 7; if (b_) { double o_; BC_V(o_, b_, Lb_, gh_expr) Lb_ = o_; } }
  // z words of a stage plane (uniform): face codes of the three components (bits 0..11), stage-D code (24..27); premod lo (0..11) / hi (12..23)
  #define ZF_WORD(k, kc, zf) { zf = 0u; if (BC && (k) == (kc)) {                                                                  \
      if ((k) == F.lo[2]) { for (int c_ = 0; c_ < 3; c_++) zf |= (unsigned)vp_code_B(F.phys[2][0], 2, 0, c_, F.outlet2d) << (4 * c_); zf |= (unsigned)vp_code_D(F.phys[2][0], 0) << 24; } \
      if ((k) == KT) { for (int c_ = 0; c_ < 3; c_++) { const int cd_ = vp_code_B(F.phys[2][1], 2, 1, c_, F.outlet2d); if (cd_) zf |= (unsigned)(cd_ | 8) << (4 * c_); }             \
                       const int cd_ = vp_code_D(F.phys[2][1], 1); if (cd_) zf |= (unsigned)(cd_ | 8) << 24; } } }
  #define ZP_WORD(kc, zp) { zp = 0u; if (BC) {                                                                                     \
      if ((kc) == F.lo[2]) for (int c_ = 0; c_ < 3; c_++) zp |= (unsigned)vp_code_B(F.phys[2][0], 2, 0, c_, F.outlet2d) << (4 * c_);           \
      if ((kc) == F.hi[2]) for (int c_ = 0; c_ < 3; c_++) zp |= (unsigned)vp_code_B(F.phys[2][1], 2, 1, c_, F.outlet2d) << (12 + 4 * c_); } }
  struct VRaw { double u[3], sx[3], sy[3], sz[3], f[3]; } N;
  #define V_LOAD {                                                                                                \
      _Pragma("unroll") for (int c = 0; c < 3; c++) {                                                              \
        N.u[c] = ldd(pu + c * F.sc_u, 0u); N.sx[c] = ldd(ps0 + c * F.sc_sl, 0u); N.sy[c] = ldd(ps1 + c * F.sc_sl, 0u); \
        N.sz[c] = ldd(ps2 + c * F.sc_sl, 0u); N.f[c] = ldd(pf + c * F.sc_f, 0u); } }
  #define V_ADVANCE(kn) { const int kc_ = min(max((kn), KB), KT);                                                 \
      if (kc_ != kcur) { pu += F.sp_u; ps0 += F.sp_sl; ps1 += F.sp_sl; ps2 += F.sp_sl; pf += F.sp_f; kcur = kc_; } }
  double fa[3] = { 0.0, 0.0, 0.0 }, fb[3] = { 0.0, 0.0, 0.0 };       // dt/2 force of planes kk-1, kk-2 (stage D adds it when !use_minion)
  const bool minion = SP != SP_RT ? (SP & SP_MINION) != 0 : F.use_minion != 0;
  // one plane of the march (see mk_F_m_body).  PH_EDGE: stages C and D and the stores tested per plane; PH_STEADY: all of them known to run
  auto plane = [&](auto ph, const int kk) __attribute__((always_inline)) {
    constexpr bool STEADY = decltype(ph)::value == PH_STEADY;
    // ---------------- plane kk: loads, bases ----------------
    double uc[3], Lb[3][3], Rb[3][3], ft[3];
    {
      V_LOAD  V_ADVANCE(kk + 1)
      #pragma unroll
      for (int c = 0; c < 3; c++) { uc[c] = N.u[c]; ft[c] = F.dt2 * N.f[c]; }
      const double *sl[3] = { N.sx, N.sy, N.sz };
      #pragma unroll
      for (int d = 0; d < 3; d++) {
        double cfl_l;
        if (d == 1) cfl_l = F.dt2 * fmax(0.0, DIVDX(uc[d], 1));       // velpred.f90:2108: division inside max()
        else cfl_l = DIVDX(F.dt2 * fmax(0.0, uc[d]), d);
        const double cfl_r = DIVDX(F.dt2 * fmin(0.0, uc[d]), d);
        #pragma unroll
        for (int c = 0; c < 3; c++) {
          Lb[d][c] = uc[c] + (0.5 - cfl_l) * sl[d][c];
          Rb[d][c] = uc[c] - (0.5 + cfl_r) * sl[d][c];
          if (minion) { Lb[d][c] = Lb[d][c] + ft[c]; Rb[d][c] = Rb[d][c] + ft[c]; }
        }
      }
    }
    // values of the next row written in the previous iteration: read before this iteration overwrites them
    double uiy_up[3], xcy_up[2];
    #pragma unroll
    for (int c = 0; c < 3; c++) uiy_up[c] = LP(lUI[c]);
    xcy_up[0] = LP(lXC[0]); xcy_up[1] = LP(lXC[1]);
    // ---------------- stage B, plane kk ----------------
    double ui0[3][3];
    {
      const int k = kk, kc = min(max(k, KB), KT);
      unsigned zf; ZF_WORD(k, kc, zf)
      #pragma unroll
      for (int c = 0; c < 3; c++) LS(lB[c]) = Lb[1][c];
      __syncthreads();
      double Lx[3], Ly[3], Lzc[3], Rx[3], Ry[3], Rz[3];
      #pragma unroll
      for (int c = 0; c < 3; c++) {
        Lx[c] = shfl_prev(Lb[0][c]); Ly[c] = LM(lB[c]); Lzc[c] = LzB[c]; LzB[c] = Lb[2][c];
        Rx[c] = Rb[0][c]; Ry[c] = Rb[1][c]; Rz[c] = Rb[2][c];
      }
      if (BC && k == kc) {
        unsigned w = wf; asm volatile("" : "+v"(w));
        if (w & 0xFFFFFFu) {
          #pragma unroll
          for (int c = 0; c < 3; c++) {
            PAIR_BC(Lx[c], Rx[c], w >> (4 * c), uc[c], U_AT(kc, -8L, c))
            PAIR_BC(Ly[c], Ry[c], w >> (12 + 4 * c), uc[c], U_AT(kc, -F.u_row, c))
          }
        }
        if ((zf & 0xFFFu) && ing_ij) {
          #pragma unroll
          for (int c = 0; c < 3; c++) PAIR_BC(Lzc[c], Rz[c], zf >> (4 * c), uc[c], U_AT(kc - 1, 0L, c))
        }
      }
      vpf_emit<0>(ui0[0], Lx, Rx, eps); vpf_emit<1>(ui0[1], Ly, Ry, eps); vpf_emit<2>(ui0[2], Lzc, Rz, eps);
      #pragma unroll
      for (int c = 0; c < 3; c++) LS(lUI[c]) = ui0[1][c];      // read by the row below at the top of the next iteration
    }
    // ---------------- stage C, plane kk-1 ----------------
    double xc1[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 }, sm1[3] = { 0.0, 0.0, 0.0 };
    if (STEADY || kk - 1 >= k0 - 1) {
      const int k = kk - 1, kc = min(max(k, KB), KT);
      unsigned zf, zp; ZF_WORD(k, kc, zf) ZP_WORD(kc, zp)
      // w0[O][c] = ui1[O][c]; w1[O][c]: the upper O-face
      double w1[3][3];
      #pragma unroll
      for (int c = 0; c < 3; c++) { w1[0][c] = lane_next(ui1[0][c]); w1[1][c] = uiy_up[c]; w1[2][c] = ui0[2][c]; }
      double Lc[3][3], Rc[3][3];
      #pragma unroll
      for (int d = 0; d < 3; d++) for (int c = 0; c < 3; c++) { Lc[d][c] = Lb1[d][c]; Rc[d][c] = Rb1[d][c]; }
      unsigned wfc = 0;
      if (BC) {
        unsigned px = wpx, py = wpy; asm volatile("" : "+v"(px)); asm volatile("" : "+v"(py));
        wfc = wf; asm volatile("" : "+v"(wfc));
        if (px | py) {
          #pragma unroll
          for (int c = 0; c < 3; c++) {
            PREMOD(Lc[0][c], Rc[0][c], px >> (4 * c), px >> (12 + 4 * c), U_AT(kc, -8L, c), U_AT(kc, 8L, c))
            PREMOD(Lc[1][c], Rc[1][c], py >> (4 * c), py >> (12 + 4 * c), U_AT(kc, -F.u_row, c), U_AT(kc, F.u_row, c))
          }
        }
        if (zp) {
          #pragma unroll
          for (int c = 0; c < 3; c++) PREMOD(Lc[2][c], Rc[2][c], zp >> (4 * c), zp >> (12 + 4 * c), U_AT(kc - 1, 0L, c), U_AT(kc + 1, 0L, c))
        }
      }
      double t[3][3];
      #pragma unroll
      for (int O = 0; O < 3; O++) {
        sm1[O] = w1[O][O] + ui1[O][O];
        #pragma unroll
        for (int C = 0; C < 3; C++) t[C][O] = F.tC[O] * sm1[O] * (w1[O][C] - ui1[O][C]);
      }
      double VL[3][2], VR[3][2];
      VL[0][0] = Lc[0][1] - t[1][2]; VR[0][0] = Rc[0][1] - t[1][2];   // D=0 C=1 O=2
      VL[0][1] = Lc[0][2] - t[2][1]; VR[0][1] = Rc[0][2] - t[2][1];   // D=0 C=2 O=1
      VL[1][0] = Lc[1][0] - t[0][2]; VR[1][0] = Rc[1][0] - t[0][2];   // D=1 C=0 O=2
      VL[1][1] = Lc[1][2] - t[2][0]; VR[1][1] = Rc[1][2] - t[2][0];   // D=1 C=2 O=0
      VL[2][0] = Lc[2][0] - t[0][1]; VR[2][0] = Rc[2][0] - t[0][1];   // D=2 C=0 O=1
      VL[2][1] = Lc[2][1] - t[1][0]; VR[2][1] = Rc[2][1] - t[1][0];   // D=2 C=1 O=0
      LS(lC[0]) = VL[1][0]; LS(lC[1]) = VL[1][1];
      __syncthreads();
      double L[3][2];
      L[0][0] = shfl_prev(VL[0][0]); L[0][1] = shfl_prev(VL[0][1]);
      L[1][0] = LM(lC[0]); L[1][1] = LM(lC[1]);
      L[2][0] = LzC[0]; L[2][1] = LzC[1];
      LzC[0] = VL[2][0]; LzC[1] = VL[2][1];
      if (BC && k == kc) {
        // components: x-faces carry C = 1, 2; y-faces C = 0, 2; z-faces C = 0, 1 (own value for a hi face: the cell's u, re-read)
        if (wfc & 0xFFFFFFu) {
          PAIR_BC(L[0][0], VR[0][0], wfc >> 4, U_AT(kc, 0L, 1), U_AT(kc, -8L, 1)) PAIR_BC(L[0][1], VR[0][1], wfc >> 8, U_AT(kc, 0L, 2), U_AT(kc, -8L, 2))
          PAIR_BC(L[1][0], VR[1][0], wfc >> 12, U_AT(kc, 0L, 0), U_AT(kc, -F.u_row, 0)) PAIR_BC(L[1][1], VR[1][1], wfc >> 20, U_AT(kc, 0L, 2), U_AT(kc, -F.u_row, 2))
        }
        if ((zf & 0xFFFu) && ing_ij) {
          PAIR_BC(L[2][0], VR[2][0], zf, U_AT(kc, 0L, 0), U_AT(kc - 1, 0L, 0)) PAIR_BC(L[2][1], VR[2][1], zf >> 4, U_AT(kc, 0L, 1), U_AT(kc - 1, 0L, 1))
        }
      }
      // XC index n: 0 = (C0,D1) 1 = (C0,D2) 2 = (C1,D0) 3 = (C1,D2) 4 = (C2,D0) 5 = (C2,D1); the advecting velocity is UI[D][D] of the lower face
      xc1[2] = vp_up(ui1[0][0], L[0][0], VR[0][0], eps); xc1[4] = vp_up(ui1[0][0], L[0][1], VR[0][1], eps);
      xc1[0] = vp_up(ui1[1][1], L[1][0], VR[1][0], eps); xc1[5] = vp_up(ui1[1][1], L[1][1], VR[1][1], eps);
      xc1[1] = vp_up(ui1[2][2], L[2][0], VR[2][0], eps); xc1[3] = vp_up(ui1[2][2], L[2][1], VR[2][1], eps);
      LS(lXC[0]) = xc1[0]; LS(lXC[1]) = xc1[5];           // the y-face fields: read by the row below at the top of the next iteration
    } else {
      __syncthreads();                                              // keeps lB / lUI single-buffered while stage C is idle (start of a chunk)
    }
    // ---------------- stage D, plane kk-2 ----------------
    if (STEADY || kk - 2 >= k0 - 1) {
      const int k = kk - 2, kc = min(max(k, KB), KT);
      unsigned zf, zp; ZF_WORD(k, kc, zf) ZP_WORD(kc, zp)
      const bool vz = k >= F.lo[2] && k <= F.hi[2];
      double Ld[3] = { LbD[0], LbD[1], LbD[2] }, Rd[3] = { RbD[0], RbD[1], RbD[2] };
      unsigned wfd = 0;
      if (BC) {
        unsigned px = wpx, py = wpy; asm volatile("" : "+v"(px)); asm volatile("" : "+v"(py));
        wfd = wf; asm volatile("" : "+v"(wfd));
        if (px | py) {
          PREMOD(Ld[0], Rd[0], px, px >> 12, U_AT(kc, -8L, 0), U_AT(kc, 8L, 0))
          PREMOD(Ld[1], Rd[1], py >> 4, py >> 16, U_AT(kc, -F.u_row, 1), U_AT(kc, F.u_row, 1))
        }
        if (zp) { PREMOD(Ld[2], Rd[2], zp >> 8, zp >> 20, U_AT(kc - 1, 0L, 2), U_AT(kc + 1, 0L, 2)) }
      }
      // XC on the upper faces: n0, n5 (y-faces) from the next row, n2, n4 (x-faces) from the next lane, n1, n3 (z-faces) from stage C above
      const double x1[6] = { xcy_up[0], xc1[1], lane_next(xc2[2]), xc1[3], lane_next(xc2[4]), xcy_up[1] };
      const double (&x0)[6] = xc2;
      const double (&g)[3] = sm2;
      double VL[3], VR[3];
      {   // D = 0: T1 = 1 with XC(0,1) = n0,  T2 = 2 with XC(0,2) = n1
        const double a1 = F.tD[1] * g[1] * (x1[0] - x0[0]);
        const double a2 = F.tD[2] * g[2] * (x1[1] - x0[1]);
        double vl = Ld[0] - a1 - a2, vr = Rd[0] - a1 - a2;
        if (!minion) { vl = vl + fb[0]; vr = vr + fb[0]; }
        VL[0] = vl; VR[0] = vr;
      }
      {   // D = 1: T1 = 0 with XC(1,0) = n2,  T2 = 2 with XC(1,2) = n3
        const double a1 = F.tD[0] * g[0] * (x1[2] - x0[2]);
        const double a2 = F.tD[2] * g[2] * (x1[3] - x0[3]);
        double vl = Ld[1] - a1 - a2, vr = Rd[1] - a1 - a2;
        if (!minion) { vl = vl + fb[1]; vr = vr + fb[1]; }
        VL[1] = vl; VR[1] = vr;
      }
      {   // D = 2: T1 = 0 with XC(2,0) = n4,  T2 = 1 with XC(2,1) = n5
        const double a1 = F.tD[0] * g[0] * (x1[4] - x0[4]);
        const double a2 = F.tD[1] * g[1] * (x1[5] - x0[5]);
        double vl = Ld[2] - a1 - a2, vr = Rd[2] - a1 - a2;
        if (!minion) { vl = vl + fb[2]; vr = vr + fb[2]; }
        VL[2] = vl; VR[2] = vr;
      }
      LS(lD) = VL[1];
      __syncthreads();
      const double Lx = shfl_prev(VL[0]), Ly = LM(lD), Lzc = LzD;
      LzD = VL[2];
      if (STEADY || k >= k0) {
        if (own_ij) {
          double e0 = vpf_riemann(Lx, VR[0], eps), e1 = vpf_riemann(Ly, VR[1], eps), e2 = vpf_riemann(Lzc, VR[2], eps);
          if (BC) {
            if (wfd >> 24) { OUT_BC(e0, wfd >> 24, Lx, VR[0], U_AT(kc, 0L, 0), U_AT(kc, -8L, 0)) OUT_BC(e1, wfd >> 28, Ly, VR[1], U_AT(kc, 0L, 1), U_AT(kc, -F.u_row, 1)) }
            if (zf >> 24) { OUT_BC(e2, zf >> 24, Lzc, VR[2], U_AT(kc, 0L, 2), U_AT(kc - 1, 0L, 2)) }
          }
          if (vy && vz) std_(qu, 0u, e0);
          if (vx && vz) std_(qv, 0u, e1);
          if (vx && vy) std_(qw, 0u, e2);
        }
        qu += F.sq[0]; qv += F.sq[1]; qw += F.sq[2];
      }
    } else {
      __syncthreads();
    }
    // hand the planes on
    #pragma unroll
    for (int d = 0; d < 3; d++) { LbD[d] = Lb1[d][d]; RbD[d] = Rb1[d][d]; sm2[d] = sm1[d]; fb[d] = fa[d]; fa[d] = ft[d]; }
    #pragma unroll
    for (int n = 0; n < 6; n++) xc2[n] = xc1[n];
    #pragma unroll
    for (int d = 0; d < 3; d++) for (int c = 0; c < 3; c++) { Lb1[d][c] = Lb[d][c]; Rb1[d][c] = Rb[d][c]; ui1[d][c] = ui0[d][c]; }
  };
  // Stage C starts at kk = k0, stage D at k0 + 1 and the stores at k0 + 2 (loads never stop): the four warm-up planes test that, every later plane runs
  // with all three compiled in.  Three barriers per plane in both forms -- the idle stages of the warm-up planes keep theirs.
  int kk = k0 - 2;
  for (; kk <= k0 + 1; kk++) plane(std::integral_constant<int, PH_EDGE>{}, kk);
  for (; kk <= k1 + 2; kk++) plane(std::integral_constant<int, PH_STEADY>{}, kk);
  #undef U_AT
  #undef BC_V
  #undef PAIR_BC
  #undef OUT_BC
  #undef PREMOD
  #undef ZF_WORD
  #undef ZP_WORD
  #undef V_LOAD
  #undef V_ADVANCE
}
// (the interior / boundary workgroup dispatch of kk_mk_F_m was measured here too: 1.198 -> 1.227 ms, not kept)
template <bool BC = true, bool INL = true, bool PW2 = false, int SP = SP_RT> __global__ void __launch_bounds__(64 * TNY) kk_vp_F_m(VArgs F, Range3 r, int klen, const double *umax) {
  int bx_, by_, bz_; xcd_remap(bx_, by_, bz_);
  vp_F_m_body<BC, INL, PW2, false, SP>(F, r, klen, umax, bx_, by_, bz_);
}
// the remainder tile column in narrow segments inside the same launch (see kk_mk_F_mc)
template <bool BC, bool INL, bool PW2, int SP = SP_RT> __global__ void __launch_bounds__(64 * TNY) kk_vp_F_mc(VArgs F, Range3 r, int klen, const double *umax, int full, int segw) {
  int bx_, by_, bz_; xcd_remap(bx_, by_, bz_);
  // GOD_COL's map in this kernel's own text (expanded from the header it costs both instantiations two VGPRs): the same origin, cut and early exit, to be
  // changed with it -- tests/cpp/godunov_plan_check.cpp holds GOD_COL, tests/test_godunov_phases_gpu.py this kernel against the face-centred stages
  Range3 rr = r;
  if (bx_ == full) {
    rr.lo[0] = r.lo[0] + full * FNX;
    if (by_ * (TNY * (64 / segw) - 2) > r.hi[1] - r.lo[1]) return;
    vp_F_m_body<BC, INL, PW2, true, SP>(F, rr, klen, umax, 0, by_, bz_, segw);
  } else {
    rr.hi[0] = r.lo[0] + full * FNX - 1;
    vp_F_m_body<BC, INL, PW2, false, SP>(F, rr, klen, umax, bx_, by_, bz_);
  }
}
static bool vfused_args(VArgs &F, const GArgs &A, const FV &u, const FV sl[3], const FV &force, const FV &um, const FV &vm, const FV &wm) {
  if (!same_geom(sl[0], sl[1]) || !same_geom(sl[0], sl[2]) || sl[0].sc != sl[1].sc || sl[0].sc != sl[2].sc) return false;
  const int KB = A.lo[2] - 1;
  const FV *in[5] = { &u, &sl[0], &sl[1], &sl[2], &force };
  for (int f = 0; f < 5; f++) if (KB < in[f]->a2 || A.hi[2] + 1 >= in[f]->a2 + in[f]->n2) return false;      // the clamped planes must exist
  F.pu = (const char *)(u.p + (long)u.n0 * u.n1 * (KB - u.a2)); F.sc_u = 8L * u.sc; F.sp_u = 8L * u.n0 * u.n1; F.g_u = FGeo{ u.a0, u.a1, u.n0 };
  for (int d = 0; d < 3; d++) F.psl[d] = (const char *)(sl[d].p + (long)sl[d].n0 * sl[d].n1 * (KB - sl[d].a2));
  F.sc_sl = 8L * sl[0].sc; F.sp_sl = 8L * sl[0].n0 * sl[0].n1; F.g_sl = FGeo{ sl[0].a0, sl[0].a1, sl[0].n0 };
  F.pf = (const char *)(force.p + (long)force.n0 * force.n1 * (KB - force.a2)); F.sc_f = 8L * force.sc; F.sp_f = 8L * force.n0 * force.n1; F.g_f = FGeo{ force.a0, force.a1, force.n0 };
  const FV *out[3] = { &um, &vm, &wm };
  for (int f = 0; f < 3; f++) {
    const FV &v = *out[f];
    F.q[f] = (char *)(v.p + (long)v.n0 * v.n1 * (KB - v.a2)); F.sq[f] = 8L * v.n0 * v.n1; F.h[f] = FGeo{ v.a0, v.a1, v.n0 };
  }
  F.u_row = 8L * u.n0;
  const double dt2 = 0.5 * A.dt, dt4 = A.dt / 4.0, dt6 = A.dt / 6.0;
  F.dt2 = dt2;
  for (int d = 0; d < 3; d++) {
    F.dx[d] = A.dx[d]; F.idx[d] = 1.0 / A.dx[d]; F.tC[d] = dt6 / A.dx[d]; F.tD[d] = dt4 / A.dx[d];
    F.lo[d] = A.lo[d]; F.hi[d] = A.hi[d]; F.phys[d][0] = A.phys[d][0]; F.phys[d][1] = A.phys[d][1];
  }
  F.use_minion = A.use_minion; F.outlet2d = A.outlet2d;
  F.p2 = (is_pow2(A.dx[0]) && is_pow2(A.dx[1]) && is_pow2(A.dx[2]) && sw().god_p2) ? 1 : 0;
  return true;
}

struct VBatchD { VArgs F; Range3 r; int klen; const double *umax; int g[3], segw; };      // segw: lanes of a row segment (NAR launches; seg_geo)
template <bool BC, bool INL, bool PW2 = false, bool NAR = false> __global__ void __launch_bounds__(64 * TNY) kk_vp_F_mb(const VBatchD *descs, const int *start, int nbox) {
  BATCH_LOCATE(VBatchD, g)
  vp_F_m_body<BC, INL, PW2, NAR>(q.F, q.r, q.klen, q.umax, BX, BY, BZ, q.segw);
}

// ====================================================================================================
// dm = 2 (BASELINE.json configs[0], the reference's CPU-runnable case): velpred_2d (velpred.f90:125-524) and mkflux_2d
// (mkflux.f90:152-691).  Two stages only -- the transverse terms use the stage-B states directly.  One thread per cell
// of the grown box, plane k = 0; fabs of a 2-D run are one z-plane on the device (z-ghost planes exist but are unused).
// ====================================================================================================
// velpred_2d pair on the lower D-face (D = 0, 1) of cell (i,j): NB every CFL factor divides INSIDE max()/min()
// (velpred.f90:255-261, 332-338), unlike velpred_3d
template <int D> DEVI void vp2_pair(const GArgs &A, const FV &u, const FV &slp, const FV &force, int i, int j, double L[2], double R[2]) {
  const double dt2 = 0.5 * A.dt;
  const double ul = ld<D>(u, i, j, 0, -1, D), ur = fv_get(u, i, j, 0, D);
  const double cl = dt2 * fmax(0.0, ul / A.dx[D]), cr = dt2 * fmin(0.0, ur / A.dx[D]);
  #pragma unroll
  for (int c = 0; c < 2; c++) {
    L[c] = ld<D>(u, i, j, 0, -1, c) + (0.5 - cl) * ld<D>(slp, i, j, 0, -1, c);
    R[c] = fv_get(u, i, j, 0, c) - (0.5 + cr) * fv_get(slp, i, j, 0, c);
    if (A.use_minion) { L[c] = L[c] + dt2 * ld<D>(force, i, j, 0, -1, c); R[c] = R[c] + dt2 * fv_get(force, i, j, 0, c); }
  }
  const int side = face_side<D>(A, i, j, 0);
  if (side >= 0) {
    #pragma unroll
    for (int c = 0; c < 2; c++) bc_pair(L[c], R[c], A.phys[D][side], side, true, c == D, (side == 0) ? ld<D>(u, i, j, 0, -1, c) : fv_get(u, i, j, 0, c), false);
  }
}
DEVI double riemann0(double L, double R, double eps) {
  const double uavg = 0.5 * (L + R);
  const bool test = ((L <= 0.0 && R >= 0.0) || (fabs(L + R) < eps));
  double un = (uavg > 0.0) ? L : R;
  return test ? 0.0 : un;
}
// UI: [0] uimhx(.,1) (normal), [1] uimhx(.,2), [2] uimhy(.,1), [3] uimhy(.,2) (normal)
__global__ void __launch_bounds__(256) kk_vp2_B(FV u, FV sl0, FV sl1, FV force, FV UI, GArgs A, Range3 r, const double *umax) {
  THREAD_IJK(r)
  if (!in_range) return;
  const double eps = eps_from(umax);
  double L[2], R[2];
  if (i >= A.lo[0]) {
    vp2_pair<0>(A, u, sl0, force, i, j, L, R);
    const double un = riemann0(L[0], R[0], eps);
    fv_at(UI, i, j, 0, 0) = un;
    const double v = (un > 0.0) ? L[1] : R[1], av = 0.5 * (L[1] + R[1]);
    fv_at(UI, i, j, 0, 1) = (fabs(un) < eps) ? av : v;
  }
  if (j >= A.lo[1]) {
    vp2_pair<1>(A, u, sl1, force, i, j, L, R);
    const double un = riemann0(L[1], R[1], eps);
    fv_at(UI, i, j, 0, 3) = un;
    const double v = (un > 0.0) ? L[0] : R[0], av = 0.5 * (L[0] + R[0]);
    fv_at(UI, i, j, 0, 2) = (fabs(un) < eps) ? av : v;
  }
}
// the MAC velocities (velpred.f90:402-443 vmac, 455-496 umac)
template <int D> DEVI void vp2_D_one(const GArgs &A, const FV &u, const FV &slp, const FV &force, const FV &UI, const FV &umac, int i, int j, double eps) {
  constexpr int T = 1 - D;
  if (coord<T>(i, j, 0) > A.hi[T]) return;
  double Lv[2], Rv[2];
  vp2_pair<D>(A, u, slp, force, i, j, Lv, Rv);
  const double dt2 = 0.5 * A.dt, dt4 = A.dt / 4.0;
  // transverse data live on T-faces: normal comp UI[T*2+T'] ... index: x-faces 0 (normal), 1;  y-faces 2, 3 (normal)
  constexpr int nrm = (T == 0) ? 0 : 3, trn = (T == 0) ? 1 : 2;      // for D = 0 (T = 1): advect with uimhy(.,2) = 3, difference uimhy(.,1) = 2
  double LR[2] = { Lv[D], Rv[D] };
  #pragma unroll
  for (int sd = 0; sd < 2; sd++) {
    const int ci = i - ((sd == 0) && D == 0), cj = j - ((sd == 0) && D == 1);
    double v = LR[sd] - (dt4 / A.dx[T]) * (ld<T>(UI, ci, cj, 0, 1, nrm) + fv_get(UI, ci, cj, 0, nrm)) * (ld<T>(UI, ci, cj, 0, 1, trn) - fv_get(UI, ci, cj, 0, trn));
    if (!A.use_minion) v = v + dt2 * fv_get(force, ci, cj, 0, D);
    LR[sd] = v;
  }
  double v = riemann0(LR[0], LR[1], eps);
  const int side = face_side<D>(A, i, j, 0);
  if (side >= 0) {
    const int ph = A.phys[D][side];
    if (ph == VDN_SLIP_WALL || ph == VDN_NO_SLIP_WALL) v = 0.0;
    else if (ph == VDN_INLET) v = (side == 0) ? ld<D>(u, i, j, 0, -1, D) : fv_get(u, i, j, 0, D);
    else if (ph == VDN_OUTLET) v = (side == 0) ? fmin(LR[1], 0.0) : fmax(LR[0], 0.0);
  }
  fv_at(umac, i, j, 0) = v;
}
__global__ void __launch_bounds__(256) kk_vp2_D(FV u, FV sl0, FV sl1, FV force, FV UI, FV um, FV vm, GArgs A, Range3 r, const double *umax) {
  THREAD_IJK(r)
  if (!in_range) return;
  const double eps = eps_from(umax);
  vp2_D_one<0>(A, u, sl0, force, UI, um, i, j, eps);
  vp2_D_one<1>(A, u, sl1, force, UI, vm, i, j, eps);
}
__global__ void kk_velmax2(FV u, Range3 r, double *out) {             // velpred.f90:216-222
  REDUCE_IJ(r)
  double m = 0.0;
  if (in_ij) m = fmax(fabs(fv_get(u, i, j, 0, 0)), fabs(fv_get(u, i, j, 0, 1)));
  block_atomic_max(out, m);
}
__global__ void kk_macmax2(FV um, FV vm, GArgs A, Range3 r, double *out) {   // mkflux.f90:248-259
  REDUCE_IJ(r)
  double m = 0.0;
  if (in_ij) {
    if (j <= A.hi[1]) m = fmax(m, fabs(fv_get(um, i, j, 0)));
    if (i <= A.hi[0]) m = fmax(m, fabs(fv_get(vm, i, j, 0)));
  }
  block_atomic_max(out, m);
}
// SI: [0*nc + c] simhx, [1*nc + c] simhy
__global__ void __launch_bounds__(256) kk_mk2_B(FV s, FV sl0, FV sl1, FV um, FV vm, FV force, FV macrhs, FV SI, GArgs A, Range3 r, const double *umax) {
  THREAD_IJK(r)
  if (!in_range) return;
  const double eps = eps_from(umax);
  for (int c = 0; c < A.ncomp; c++) {
    double L, R;
    if (i >= A.lo[0]) { mk_pair<0>(A, s, sl0, um, force, macrhs, c, i, j, 0, L, R); fv_at(SI, i, j, 0, 0 * A.ncomp + c) = upwind_mac(L, R, fv_get(um, i, j, 0), eps); }
    if (j >= A.lo[1]) { mk_pair<1>(A, s, sl1, vm, force, macrhs, c, i, j, 0, L, R); fv_at(SI, i, j, 0, 1 * A.ncomp + c) = upwind_mac(L, R, fv_get(vm, i, j, 0), eps); }
  }
}
// edge states and fluxes (mkflux.f90:472-558 sedgey, 570-660 sedgex)
template <int D> DEVI void mk2_D_one(const GArgs &A, const FV &s, const FV &slp, const FV &macD, const FV &macT, const FV &force, const FV &macrhs,
                                     const FV &SI, const FV &sedge, const FV &flux, int c, int i, int j, double eps) {
  constexpr int T = 1 - D;
  if (coord<T>(i, j, 0) > A.hi[T]) return;
  double L, R;
  mk_pair<D>(A, s, slp, macD, force, macrhs, c, i, j, 0, L, R);
  const double dt2 = 0.5 * A.dt, dt4 = A.dt / 4.0;
  const bool cons = A.cons[c] != 0;
  double LR[2] = { L, R };
  #pragma unroll
  for (int sd = 0; sd < 2; sd++) {
    const int ci = i - ((sd == 0) && D == 0), cj = j - ((sd == 0) && D == 1);
    const double s0 = fv_get(s, ci, cj, 0, c);
    double v = LR[sd] - trans_term<T>(A, SI, T * A.ncomp + c, macT, cons, ci, cj, 0, dt2, dt4);
    if (cons) v = v + (dt2 / A.dx[T]) * s0 * (ld<T>(macT, ci, cj, 0, 1) - fv_get(macT, ci, cj, 0));
    if (!A.use_minion) {
      v = v + dt2 * fv_get(force, ci, cj, 0, c);
      if (cons) v = v - dt2 * s0 * fv_get(macrhs, ci, cj, 0);
    }
    LR[sd] = v;
  }
  const double um = fv_get(macD, i, j, 0);
  double e = upwind_mac(LR[0], LR[1], um, eps);
  const int side = face_side<D>(A, i, j, 0);
  if (side >= 0) {
    const int ph = A.phys[D][side];
    const double in = (side == 0) ? LR[1] : LR[0];
    const bool vel = A.is_vel != 0;
    if (ph == VDN_INLET) e = (side == 0) ? ld<D>(s, i, j, 0, -1, c) : fv_get(s, i, j, 0, c);
    else if (ph == VDN_SLIP_WALL) e = (vel && c == D) ? 0.0 : in;
    else if (ph == VDN_NO_SLIP_WALL) e = vel ? 0.0 : in;
    else if (ph == VDN_OUTLET) e = (vel && c == D) ? ((side == 0) ? fmin(in, 0.0) : fmax(in, 0.0)) : in;
  }
  fv_at(sedge, i, j, 0, c) = e;
  if (cons) fv_at(flux, i, j, 0, c) = e * um;
}
__global__ void __launch_bounds__(256) kk_mk2_D(FV s, FV sl0, FV sl1, FV um, FV vm, FV force, FV macrhs, FV SI, FV sex, FV sey, FV flx, FV fly,
                                                GArgs A, Range3 r, const double *umax) {
  THREAD_IJK(r)
  if (!in_range) return;
  const double eps = eps_from(umax);
  for (int c = 0; c < A.ncomp; c++) {
    mk2_D_one<0>(A, s, sl0, um, vm, force, macrhs, SI, sex, flx, c, i, j, eps);
    mk2_D_one<1>(A, s, sl1, vm, um, force, macrhs, SI, sey, fly, c, i, j, eps);
  }
}
static FV work_fv2(const BoxP &b) {        // one plane over [lo-1, hi+1]^2
  FV f; f.p = nullptr; f.a0 = b.lo[0] - 1; f.a1 = b.lo[1] - 1; f.a2 = 0;
  f.n0 = b.hi[0] - b.lo[0] + 3; f.n1 = b.hi[1] - b.lo[1] + 3; f.n2 = 1;
  f.sc = (long)f.n0 * f.n1;
  return f;
}
static void ranges2(const GArgs &A, Range3 &rv, Range3 &rg, Range3 &rf) {
  for (int d = 0; d < 2; d++) { rv.lo[d] = A.lo[d]; rv.hi[d] = A.hi[d]; rg.lo[d] = A.lo[d] - 1; rg.hi[d] = A.hi[d] + 1; rf.lo[d] = A.lo[d]; rf.hi[d] = A.hi[d] + 1; }
  rv.lo[2] = rv.hi[2] = rg.lo[2] = rg.hi[2] = rf.lo[2] = rf.hi[2] = 0;
}
static void k2_velpred(const vdn_multifab *u, vdn_multifab **umac, const vdn_multifab *force, const double *dx, double dt, const vdn_bc_tower *bct) {
  REQUIRE(u->nc == 2 && u->ng >= 3 && force->ng >= 1 && umac[0]->ng >= 1, "velpred (dm = 2): operand shapes");
  hipStream_t st = ctx().stream;
  for (int ib = 0; ib < u->nfabs(); ib++) {
    size_t mark = arena_mark();
    GArgs A; fill_gargs(A, u, ib, bct, 0, 2, dx, dt);
    A.is_vel = 1;
    BoxP bp = make_boxp(u, ib, bct);
    FV w = work_fv2(bp);
    const size_t fld = (size_t)w.sc * sizeof(double);
    FV sl[2] = { w, w }, UI = w;
    sl[0].p = (double *)arena_alloc(fld * 2); sl[1].p = (double *)arena_alloc(fld * 2); UI.p = (double *)arena_alloc(fld * 4);
    double *umax = (double *)arena_alloc(256);
    HIPCHK(hipMemsetAsync(umax, 0, sizeof(double), st));
    Range3 rv, rg, rf; ranges2(A, rv, rg, rf);
    hipLaunchKernelGGL(kk_velmax2, reduce_grid(rv), dim3(64, 4, 1), 0, st, u->fabs[ib], rv, umax);
    hipLaunchKernelGGL(kk_slopes, grid_for(rg), dim3(64, 4, 1), 0, st, u->fabs[ib], sl[0], sl[1], sl[1], A, rg, 3);
    hipLaunchKernelGGL(kk_vp2_B, grid_for(rg), dim3(64, 4, 1), 0, st, u->fabs[ib], sl[0], sl[1], force->fabs[ib], UI, A, rg, umax);
    hipLaunchKernelGGL(kk_vp2_D, grid_for(rf), dim3(64, 4, 1), 0, st, u->fabs[ib], sl[0], sl[1], force->fabs[ib], UI, umac[0]->fabs[ib], umac[1]->fabs[ib], A, rf, umax);
    arena_release(mark);
  }
}
static void k2_mkflux(const vdn_multifab *s, vdn_multifab **sedge, vdn_multifab **flux, vdn_multifab **umac, const vdn_multifab *force,
                      const vdn_multifab *mac_rhs, const double *dx, double dt, const vdn_bc_tower *bct, bool is_vel, int bccomp, const int *is_cons) {
  const int ncomp = s->nc;
  REQUIRE(ncomp <= 3 && s->ng >= 3 && umac[0]->ng >= 1 && force->ng >= 1 && mac_rhs->ng >= 1, "mkflux (dm = 2): operand shapes");
  hipStream_t st = ctx().stream;
  for (int ib = 0; ib < s->nfabs(); ib++) {
    size_t mark = arena_mark();
    GArgs A; fill_gargs(A, s, ib, bct, bccomp, ncomp, dx, dt);
    A.is_vel = is_vel ? 1 : 0;
    for (int c = 0; c < ncomp; c++) A.cons[c] = is_cons[c] ? 1 : 0;
    BoxP bp = make_boxp(s, ib, bct);
    FV w = work_fv2(bp);
    const size_t fld = (size_t)w.sc * sizeof(double);
    FV sl[2] = { w, w }, SI = w;
    sl[0].p = (double *)arena_alloc(fld * ncomp); sl[1].p = (double *)arena_alloc(fld * ncomp); SI.p = (double *)arena_alloc(fld * 2 * ncomp);
    double *umax = (double *)arena_alloc(256);
    HIPCHK(hipMemsetAsync(umax, 0, sizeof(double), st));
    Range3 rv, rg, rf; ranges2(A, rv, rg, rf);
    const FV &um = umac[0]->fabs[ib], &vm = umac[1]->fabs[ib];
    hipLaunchKernelGGL(kk_macmax2, reduce_grid(rf), dim3(64, 4, 1), 0, st, um, vm, A, rf, umax);
    hipLaunchKernelGGL(kk_slopes, grid_for(rg), dim3(64, 4, 1), 0, st, s->fabs[ib], sl[0], sl[1], sl[1], A, rg, 3);
    hipLaunchKernelGGL(kk_mk2_B, grid_for(rg), dim3(64, 4, 1), 0, st, s->fabs[ib], sl[0], sl[1], um, vm, force->fabs[ib], mac_rhs->fabs[ib], SI, A, rg, umax);
    hipLaunchKernelGGL(kk_mk2_D, grid_for(rf), dim3(64, 4, 1), 0, st, s->fabs[ib], sl[0], sl[1], um, vm, force->fabs[ib], mac_rhs->fabs[ib], SI,
                       sedge[0]->fabs[ib], sedge[1]->fabs[ib], flux[0]->fabs[ib], flux[1]->fabs[ib], A, rf, umax);
    arena_release(mark);
  }
}

#define GOD_X_VP_M(bc, inl, upd, pw2, sp, nar, cols) GOD_CASE(GOD_FORM(bc, inl, upd, pw2, sp, nar, cols), (kk_vp_F_m<bc, inl, pw2, sp>), F, r, G.klen, umax)
#define GOD_X_VP_MC(bc, inl, upd, pw2, sp, nar, cols) GOD_CASE(GOD_FORM(bc, inl, upd, pw2, sp, nar, cols), (kk_vp_F_mc<bc, inl, pw2, sp>), F, r, G.klen, umax, G.full, G.segw)
#define GOD_X_VP_MB(bc, inl, upd, pw2, sp, nar, cols) GOD_CASE(GOD_FORM(bc, inl, upd, pw2, sp, nar, cols), (kk_vp_F_mb<bc, inl, pw2, nar>), dd, ds, n)
static void launch_vp(const GodForm &f, const GodGrid &G, hipStream_t st, const VArgs &F, const Range3 &r, const double *umax) {
  const dim3 g(G.g[0], G.g[1], G.g[2]);
  GOD_VP_M_FORMS(GOD_X_VP_M) GOD_VP_MC_FORMS(GOD_X_VP_MC) GOD_NO_FORM("velpred");
}
static void launch_vp_b(const GodForm &f, int tot, hipStream_t st, const VBatchD *dd, const int *ds, int n) {
  const dim3 g(tot);
  GOD_VP_MB_FORMS(GOD_X_VP_MB) GOD_NO_FORM("velpred, batched");
}
void k_velpred(const vdn_multifab *u, vdn_multifab **umac, const vdn_multifab *force, const double *dx, double dt,
               const vdn_bc_tower *bct) {
  Prof prof_("velpred");
  if (ctx().prm.dm == 2) { k2_velpred(u, umac, force, dx, dt, bct); return; }
  REQUIRE(u->nc == 3 && u->ng >= 3 && force->ng >= 1 && umac[0]->ng >= 1, "velpred: operand shapes");
  hipStream_t st = ctx().stream;
  if (use_batched(u) && !sw().godunov_plain) {            // the slopes, then stages B + C + D in one march per box (vp_F_m_body)
    size_t mark = arena_mark();
    const int nb = u->nfabs();
    GodBatch<VpD> B; B.d.resize(nb);
    double *umax = (double *)arena_alloc(sizeof(double) * nb);
    HIPCHK(hipMemsetAsync(umax, 0, sizeof(double) * nb, st));
    std::vector<VBatchD> fd(nb);
    bool ok = true, inflow = false, any = false;
    for (int ib = 0; ib < nb && ok; ib++) {
      VpD &q = B.d[ib];
      const GodBox X = god_box(u, ib, bct, 0, 3, dx, dt, true, nullptr, false);
      q.A = X.A; q.sl0 = X.sl[0]; q.sl1 = X.sl[1]; q.sl2 = X.sl[2]; q.rg = X.rg; q.rf = X.rf;
      for (int d = 0; d < 3; d++) { q.rm.lo[d] = q.A.lo[d]; q.rm.hi[d] = q.A.hi[d]; }
      q.s = u->fabs[ib]; q.force = force->fabs[ib]; q.um = umac[0]->fabs[ib]; q.vm = umac[1]->fabs[ib]; q.wm = umac[2]->fabs[ib];
      q.umax = umax + ib;
      any = any || X.any; inflow = inflow || X.inflow;
      ok = vfused_args(fd[ib].F, q.A, q.s, X.sl, q.force, q.um, q.vm, q.wm);
      fd[ib].r = q.rf; fd[ib].umax = q.umax;
      batch_grid(fd[ib]);
    }
    if (ok) {
      B.finish();
      hipLaunchKernelGGL(kk_velmax_b, dim3(B.tot[1]), dim3(64, 4, 1), 0, st, B.dev, B.st[1], nb);       // per-box max |u| over the valid cells
      hipLaunchKernelGGL(kk_slopes_b<VpD>, dim3(B.tot[0]), dim3(64, 4, 1), 0, st, B.dev, B.st[0], nb, 7);
      launch_batched(fd, god_vp_form(any, inflow, fd[0].F.p2 != 0, false, false, true), st, launch_vp_b);
      arena_release(mark);
      return;
    }
    arena_release(mark);                               // a box's layouts refused: the level runs box by box
  }
  for (int ib = 0; ib < u->nfabs(); ib++) {
    size_t mark = arena_mark();
    const bool keep = (int)ctx().slope_src.size() == u->nfabs();           // advance_timestep: mkflux(uold) reuses these slopes
    const GodBox X = god_box(u, ib, bct, 0, 3, dx, dt, true, nullptr, keep);
    const GArgs &A = X.A; const FV *sl = X.sl; const Range3 &rg = X.rg, &rf = X.rf;
    if (keep) ctx().slope_src[ib] = u->fabs[ib].p;
    double *umax = (double *)arena_alloc(256);
    HIPCHK(hipMemsetAsync(umax, 0, sizeof(double), st));
    launch_slopes(u->fabs[ib], sl, A, rg, 3, umax, st);      // + max |u| (kk_velmax)
    VArgs VA;
    if (!sw().godunov_plain && vfused_args(VA, A, u->fabs[ib], sl, force->fabs[ib], umac[0]->fabs[ib], umac[1]->fabs[ib], umac[2]->fabs[ib])) {
      const Ext3 e(rf);             // stages B + C + D in one march, boundary rules inside (see vp_F_m_body)
      const GodGrid gF = god_grid_tiles(e.n[0], e.n[1], e.n[2], sw().fused_kchunks);
      GodGrid gM = gF;
      const bool cols = god_grid_cols(e.n[0], e.n[1], e.n[2], sw().god_narrow, gM);
      const GodForm f = god_vp_form(X.any, X.inflow, VA.p2 != 0, VA.use_minion != 0, cols, false);
      launch_vp(f, f.cols ? gM : gF, st, VA, rf, umax);
    } else {                       // the face-centred stages: VDN_GODUNOV_PLAIN, or field layouts the fused march refuses
      FV UI = X.w, XC = X.w;
      UI.p = (double *)arena_alloc(X.fld * 9);
      XC.p = (double *)arena_alloc(X.fld * 6);
      hipLaunchKernelGGL(kk_vp_B, grid_for(rg), dim3(64, 4, 1), 0, st, u->fabs[ib], sl[0], sl[1], sl[2], force->fabs[ib], UI, A, rg, umax);
      hipLaunchKernelGGL(kk_vp_C, grid_for(rg), dim3(64, 4, 1), 0, st, u->fabs[ib], sl[0], sl[1], sl[2], force->fabs[ib], UI, XC, A, rg, umax);
      hipLaunchKernelGGL(kk_vp_D, grid_for(rf), dim3(64, 4, 1), 0, st, u->fabs[ib], sl[0], sl[1], sl[2], force->fabs[ib], UI, XC,
                         umac[0]->fabs[ib], umac[1]->fabs[ib], umac[2]->fabs[ib], A, rf, umax);
    }
    arena_release(mark);
  }
}
