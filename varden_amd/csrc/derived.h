// derived.h -- the derived cell quantities of src/makevort.f90 as device VALUES: the vorticity and the velocity magnitude of one cell of a box.
// One restatement, two readers: make_vorticity / make_magvel store the value into a multifab (pointwise.hip: vort_K, magvel_K), tagging by criteria
// compares it with its thresholds without storing it (grids.hip: kk_tag_by).  Every file is built with -ffp-contract=off, so the two readers see the
// same bits.
#pragma once
#include "vdn_dev.h"

struct VortArgs { int lo[3], hi[3]; int phys[3][2]; double dx[3]; int comp, dm; };
// d(u_c)/dx_D: centred (uycen & co., makevort.f90:568-572), one-sided next to an inflow / no-slip face (uylo / uyhi, :574-584)
template <int D> DEVI double vort_der(const FV &u, int c, int side, int i, int j, int k, double dxd) {
  const double up = fv_get(u, i + (D == 0), j + (D == 1), k + (D == 2), c), u0 = fv_get(u, i, j, k, c), um = fv_get(u, i - (D == 0), j - (D == 1), k - (D == 2), c);
  if (side < 0) return (up + 3.0 * u0 - 4.0 * um) / (3.0 * dxd);
  if (side > 0) return -(um + 3.0 * u0 - 4.0 * up) / (3.0 * dxd);
  return 0.5 * (up - um) / dxd;
}
DEVI bool vort_fix3(int p) { return p == VDN_INLET || p == VDN_NO_SLIP_WALL; }                           // makevort.f90:188-195
DEVI bool vort_fix2(int p) { return p == VDN_INLET || p == VDN_SLIP_WALL || p == VDN_NO_SLIP_WALL; }     // makevort.f90:116-117
DEVI double vort_value(const FV &u, const VortArgs &A, int i, int j, int k) {
  if (A.dm == 2) {
    // makevort_2d (makevort.f90:93-156; k = 0 in a dm = 2 run, every plane of a z-uniform copy for make_vorticity_plane): one-sided forms over dx (not 3 dx), slip walls included; the y-face loops run last and
    // overwrite, so at a corner the x derivative is the centred one
    double vx = (fv_get(u, i + 1, j, k, 1) - fv_get(u, i - 1, j, k, 1)) / (2.0 * A.dx[0]);
    double uy = (fv_get(u, i, j + 1, k, 0) - fv_get(u, i, j - 1, k, 0)) / (2.0 * A.dx[1]);
    const bool ylo = j == A.lo[1] && vort_fix2(A.phys[1][0]), yhi = j == A.hi[1] && vort_fix2(A.phys[1][1]);
    if (!(ylo || yhi)) {
      if (i == A.lo[0] && vort_fix2(A.phys[0][0])) vx = (fv_get(u, i + 1, j, k, 1) + 3.0 * fv_get(u, i, j, k, 1) - 4.0 * fv_get(u, i - 1, j, k, 1)) / A.dx[0];
      if (i == A.hi[0] && vort_fix2(A.phys[0][1])) vx = -(fv_get(u, i - 1, j, k, 1) + 3.0 * fv_get(u, i, j, k, 1) - 4.0 * fv_get(u, i + 1, j, k, 1)) / A.dx[0];
    }
    if (ylo) uy = (fv_get(u, i, j + 1, k, 0) + 3.0 * fv_get(u, i, j, k, 0) - 4.0 * fv_get(u, i, j - 1, k, 0)) / A.dx[1];
    if (yhi) uy = -(fv_get(u, i, j - 1, k, 0) + 3.0 * fv_get(u, i, j, k, 0) - 4.0 * fv_get(u, i, j + 1, k, 0)) / A.dx[1];
    return vx - uy;
  }
  // makevort_3d (makevort.f90:158-682): faces, edges and corners follow one rule per direction
  const int q[3] = { i, j, k };
  int side[3];
  #pragma unroll
  for (int d = 0; d < 3; d++) {
    side[d] = 0;
    if (q[d] == A.lo[d] && vort_fix3(A.phys[d][0])) side[d] = -1;
    if (q[d] == A.hi[d] && vort_fix3(A.phys[d][1])) side[d] = 1;
  }
  const double uy = vort_der<1>(u, 0, side[1], i, j, k, A.dx[1]), uz = vort_der<2>(u, 0, side[2], i, j, k, A.dx[2]);
  const double vx = vort_der<0>(u, 1, side[0], i, j, k, A.dx[0]), vz = vort_der<2>(u, 1, side[2], i, j, k, A.dx[2]);
  const double wx = vort_der<0>(u, 2, side[0], i, j, k, A.dx[0]), wy = vort_der<1>(u, 2, side[1], i, j, k, A.dx[1]);
  return sqrt((wy - vz) * (wy - vz) + (uz - wx) * (uz - wx) + (vx - uy) * (vx - uy));     // vorfun, :676-680
}
DEVI double magvel_value(const FV &u, int dm, int i, int j, int k) {                                    // makevort.f90:684-724
  double s = fv_get(u, i, j, k, 0) * fv_get(u, i, j, k, 0) + fv_get(u, i, j, k, 1) * fv_get(u, i, j, k, 1);
  if (dm == 3) s = s + fv_get(u, i, j, k, 2) * fv_get(u, i, j, k, 2);
  return sqrt(s);
}
// the box description vort_value reads: valid box, physical sides, spacings of the `rule` (2 or 3) directions that take part
static inline VortArgs vort_args(const vdn_multifab *u, int i, const vdn_bc_tower *bct, const double *dx, int rule, int comp) {
  VortArgs A; const BoxP bp = make_boxp(u, i, bct);
  for (int d = 0; d < 3; d++) { A.lo[d] = bp.lo[d]; A.hi[d] = bp.hi[d]; A.dx[d] = d < rule ? dx[d] : 1.0;
    for (int s = 0; s < 2; s++) A.phys[d][s] = bp.phys[d][s]; }
  A.comp = comp; A.dm = rule;
  return A;
}
