// iso_cell.h -- one cell of vdn_isosurface (iso.hip; include/varden_amd.h states the definitions): nodes -> masks -> triangles, area, volume.  No HIP, no library type:
// hipcc compiles it for the kernels, plain g++ for tests/cpp/iso_cell_check.cpp, and the tests restate it in numpy.  The case table exists here and nowhere else.
//
// Nodes.  a[27] is the 3 x 3 x 3 neighbourhood of the cell, a[(di + 1) + 3 (dj + 1) + 9 (dk + 1)].  Corner c = cx + 2 cy + 4 cz of the cell is node (i + cx, j + cy, k + cz);
// its value is a pairwise mean m = 0.5 a + 0.5 b along x, then along y, then along z (iso_nodes).  flo[d] / fhi[d]: the cell's low / high nodes along d lie on a domain
// face whose ghost cell holds the value ON the face (EXT_DIR): m is then the ghost value alone.
// Tetrahedra.  Six Kuhn tetrahedra around the diagonal corner 0 -- corner 7, tetrahedron n = 0 .. 5 for the axis orders (a, b, c) = (x,y,z), (x,z,y), (y,x,z), (y,z,x), (z,x,y),
// (z,y,x): v0 = corner 0, v1 = v0 + e_a, v2 = v1 + e_b, v3 = corner 7.  det(v1 - v0, v2 - v0, v3 - v0) has the sign of the permutation: + for n = 0, 3, 4.
// Above.  A vertex is above when q > iso.  An edge is crossed between a not-above end A and an above end B: t = (iso - q_A) / (q_B - q_A), p_d = x_A,d + t (x_B,d - x_A,d),
// always from A to B, so every tetrahedron (and every cell of a level) that shares the edge forms the same bits.
// Cases, by the number of vertices above (mask: bit v set = vertex v above):
//   0       nothing.                                        4   V_tet.
//   1 or 3  the lone vertex L (the one above, or the one not above) and the others (o1, o2, o3), which make (L, o1, o2, o3) an even permutation of (0, 1, 2, 3):
//           L = 0: (1, 2, 3), L = 1: (0, 3, 2), L = 2: (0, 1, 3), L = 3: (0, 2, 1).  P_i crosses the edge L -- o_i, t_i is its t.  One triangle (P1, P2, P3); P2 and P3 change
//           places when (the tetrahedron is positive) != (L is above).  Volume above: L above: ((V_tet (1 - t1)) (1 - t2)) (1 - t3); L not above: V_tet - ((V_tet t1) t2) t3.
//   2       A1 < A2 above, B1 < B2 not above; P_rs crosses B_r -- A_s, t_rs is its t.  Two triangles (P11, P12, P22), (P11, P22, P21); in each the last two change places when
//           (the tetrahedron is positive) == (the mask is none of {0, 2} and {1, 3}).  Volume above: the wedge A1 P11 P21 - A2 P12 P22 as the three tetrahedra
//           (A1, P11, P21, A2), (P11, P21, A2, P12), (P21, A2, P12, P22), each |det| / 6, which in the tetrahedron's own affine coordinates are products without a difference of
//           products: with a = 1 - t11, b = 1 - t21, c = 1 - t12, d = 1 - t22:  (((V_tet a) b) + (((V_tet t11) b) c)) + (((V_tet t21) c) d).
// With these orders (p1 - p0) x (p2 - p0) points towards the not-above side.
// Per triangle: cross = (p1 - p0) x (p2 - p0), c_x = e1_y e2_z - e1_z e2_y and cyclic; area 0.5 sqrt((c_x c_x + c_y c_y) + c_z c_z); area_vec 0.5 c_d.  Per cell every sum
// starts from +0 and takes tetrahedron 0 .. 5, triangle 0 .. 1 in order.  A cell with a non-finite node emits nothing and adds nothing.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define ISO_HD __host__ __device__ __forceinline__
#define ISO_UNROLL _Pragma("unroll")
#define ISO_NOUNROLL _Pragma("nounroll")
#else
#define ISO_HD inline
#define ISO_UNROLL
#define ISO_NOUNROLL
#endif

constexpr int ISO_NONFINITE = -1, ISO_MAX_TRI = 12;

struct IsoSums { double area, av[3], vol; };

ISO_HD bool iso_finite(double v) { return fabs(v) < __builtin_huge_val(); }
ISO_HD double iso_mean(double lo, double hi, bool face_lo, bool face_hi) { return face_lo ? lo : face_hi ? hi : 0.5 * lo + 0.5 * hi; }

ISO_HD void iso_nodes(const double (&a)[27], const bool (&flo)[3], const bool (&fhi)[3], double (&q)[8]) {
  double mx[2][3][3], my[2][2][3];
  ISO_UNROLL
  for (int kk = 0; kk < 3; kk++) {
    ISO_UNROLL
    for (int jj = 0; jj < 3; jj++) {
      mx[0][jj][kk] = iso_mean(a[0 + 3 * jj + 9 * kk], a[1 + 3 * jj + 9 * kk], flo[0], false);
      mx[1][jj][kk] = iso_mean(a[1 + 3 * jj + 9 * kk], a[2 + 3 * jj + 9 * kk], false, fhi[0]);
    }
  }
  ISO_UNROLL
  for (int kk = 0; kk < 3; kk++) {
    ISO_UNROLL
    for (int cx = 0; cx < 2; cx++) {
      my[cx][0][kk] = iso_mean(mx[cx][0][kk], mx[cx][1][kk], flo[1], false);
      my[cx][1][kk] = iso_mean(mx[cx][1][kk], mx[cx][2][kk], false, fhi[1]);
    }
  }
  ISO_UNROLL
  for (int cy = 0; cy < 2; cy++) {
    ISO_UNROLL
    for (int cx = 0; cx < 2; cx++) {
      q[cx + 2 * cy] = iso_mean(my[cx][cy][0], my[cx][cy][1], flo[2], false);
      q[cx + 2 * cy + 4] = iso_mean(my[cx][cy][1], my[cx][cy][2], false, fhi[2]);
    }
  }
}

// a node value by a run-time corner number, picked by the corner's bits from values held in registers (an indexed array would leave the registers)
ISO_HD double iso_pick8(const double (&q)[8], int c) {
  const double q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3], q4 = q[4], q5 = q[5], q6 = q[6], q7 = q[7];
  const bool x = c & 1, y = c & 2, z = c & 4;
  const double a0 = x ? q1 : q0, a1 = x ? q3 : q2, a2 = x ? q5 : q4, a3 = x ? q7 : q6;
  const double b0 = y ? a1 : a0, b1 = y ? a3 : a2;
  return z ? b1 : b0;
}
template <class T> ISO_HD T iso_pick4(T a0, T a1, T a2, T a3, int v) { return v == 0 ? a0 : v == 1 ? a1 : v == 2 ? a2 : a3; }
// corners 1 and 2 of tetrahedron n (corner 0 is cell corner 0, corner 3 is cell corner 7), whether it is positive
ISO_HD void iso_tet(int n, int &c1, int &c2, bool &positive) {
  const int a = n >> 1, r0 = a == 0 ? 1 : 0, r1 = a == 2 ? 1 : 2, b = (n & 1) ? r1 : r0;
  c1 = 1 << a; c2 = c1 | (1 << b);
  positive = n == 0 || n == 3 || n == 4;
}
ISO_HD int iso_bits4(int m) { return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1); }
ISO_HD int iso_tet_mask(const double (&q)[8], double iso, int c1, int c2) {
  return (q[0] > iso ? 1 : 0) | (iso_pick8(q, c1) > iso ? 2 : 0) | (iso_pick8(q, c2) > iso ? 4 : 0) | (q[7] > iso ? 8 : 0);
}

// the number of triangles of a cell (ISO_NONFINITE: a node is not finite): what iso_cell returns, without the geometry
ISO_HD int iso_count(const double (&q)[8], double iso) {
  bool fin = true;
  ISO_UNROLL
  for (int c = 0; c < 8; c++) fin = fin && iso_finite(q[c]);
  if (!fin) return ISO_NONFINITE;
  int n = 0;
  ISO_UNROLL
  for (int tet = 0; tet < 6; tet++) {
    int c1, c2; bool pos;
    iso_tet(tet, c1, c2, pos);
    const int nab = iso_bits4(iso_tet_mask(q, iso, c1, c2));
    n += nab == 2 ? 2 : (nab == 1 || nab == 3) ? 1 : 0;
  }
  return n;
}

// the crossing of the edge between tetrahedron vertices A (not above) and B (above); cA, cB: their cell corners
ISO_HD double iso_cross(double qA, double qB, int cA, int cB, const double (&xlo)[3], const double (&xhi)[3], double iso, double (&p)[3]) {
  const double t = (iso - qA) / (qB - qA);
  ISO_UNROLL
  for (int d = 0; d < 3; d++) {
    const double xa = ((cA >> d) & 1) ? xhi[d] : xlo[d], xb = ((cB >> d) & 1) ? xhi[d] : xlo[d];
    p[d] = xa + t * (xb - xa);
  }
  return t;
}
template <class Emit> ISO_HD void iso_tri(IsoSums &S, const double (&p0)[3], const double (&p1)[3], const double (&p2)[3], Emit &emit) {
  const double e1[3] = { p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2] }, e2[3] = { p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2] };
  const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
  S.area = S.area + 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
  S.av[0] = S.av[0] + 0.5 * cx; S.av[1] = S.av[1] + 0.5 * cy; S.av[2] = S.av[2] + 0.5 * cz;
  emit(p0, p1, p2);
}

// the whole cell: q[8] the node values, xlo / xhi the positions of its low and high nodes, vtet = dx dy dz / 6.  Calls emit(p0, p1, p2) per triangle in output order, fills S,
// returns the number of triangles or ISO_NONFINITE
template <class Emit>
ISO_HD int iso_cell(const double (&q)[8], const double (&xlo)[3], const double (&xhi)[3], double iso, double vtet, IsoSums &S, Emit &&emit) {
  S.area = 0.0; S.av[0] = 0.0; S.av[1] = 0.0; S.av[2] = 0.0; S.vol = 0.0;
  bool fin = true;
  int above = 0;
  ISO_UNROLL
  for (int c = 0; c < 8; c++) { fin = fin && iso_finite(q[c]); above += q[c] > iso ? 1 : 0; }
  if (!fin) return ISO_NONFINITE;
  if (above == 0) return 0;
  int ntri = 0;
  ISO_NOUNROLL
  for (int tet = 0; tet < 6; tet++) {
    if (above == 8) { S.vol = S.vol + vtet; continue; }
    int c1, c2; bool pos;
    iso_tet(tet, c1, c2, pos);
    const double q0 = q[0], q1 = iso_pick8(q, c1), q2 = iso_pick8(q, c2), q3 = q[7];
    const int m = (q0 > iso ? 1 : 0) | (q1 > iso ? 2 : 0) | (q2 > iso ? 4 : 0) | (q3 > iso ? 8 : 0), nab = iso_bits4(m);
    if (nab == 0) continue;
    if (nab == 4) { S.vol = S.vol + vtet; continue; }
    if (nab == 2) {
      const int A1 = (m & 1) ? 0 : (m & 2) ? 1 : 2, A2 = (m & 8) ? 3 : (m & 4) ? 2 : 1, w = ~m & 15;
      const int B1 = (w & 1) ? 0 : (w & 2) ? 1 : 2, B2 = (w & 8) ? 3 : (w & 4) ? 2 : 1;
      const double qA1 = iso_pick4(q0, q1, q2, q3, A1), qA2 = iso_pick4(q0, q1, q2, q3, A2), qB1 = iso_pick4(q0, q1, q2, q3, B1), qB2 = iso_pick4(q0, q1, q2, q3, B2);
      const int cA1 = iso_pick4(0, c1, c2, 7, A1), cA2 = iso_pick4(0, c1, c2, 7, A2), cB1 = iso_pick4(0, c1, c2, 7, B1), cB2 = iso_pick4(0, c1, c2, 7, B2);
      double p11[3], p12[3], p21[3], p22[3];
      const double t11 = iso_cross(qB1, qA1, cB1, cA1, xlo, xhi, iso, p11), t12 = iso_cross(qB1, qA2, cB1, cA2, xlo, xhi, iso, p12);
      const double t21 = iso_cross(qB2, qA1, cB2, cA1, xlo, xhi, iso, p21), t22 = iso_cross(qB2, qA2, cB2, cA2, xlo, xhi, iso, p22);
      const bool flip = pos == (m != 5 && m != 10);
      if (flip) { iso_tri(S, p11, p22, p12, emit); iso_tri(S, p11, p21, p22, emit); }
      else      { iso_tri(S, p11, p12, p22, emit); iso_tri(S, p11, p22, p21, emit); }
      const double a = 1.0 - t11, b = 1.0 - t21, c = 1.0 - t12, d = 1.0 - t22;
      S.vol = S.vol + ((((vtet * a) * b) + (((vtet * t11) * b) * c)) + (((vtet * t21) * c) * d));
      ntri += 2;
    } else {
      const bool lone_above = nab == 1;
      const int one = lone_above ? m : (~m & 15);
      const int L = (one & 1) ? 0 : (one & 2) ? 1 : (one & 4) ? 2 : 3;
      const int o1 = (0x0001 >> (4 * L)) & 15, o2 = (0x2132 >> (4 * L)) & 15, o3 = (0x1323 >> (4 * L)) & 15;
      const double qL = iso_pick4(q0, q1, q2, q3, L), qo1 = iso_pick4(q0, q1, q2, q3, o1), qo2 = iso_pick4(q0, q1, q2, q3, o2), qo3 = iso_pick4(q0, q1, q2, q3, o3);
      const int cL = iso_pick4(0, c1, c2, 7, L), co1 = iso_pick4(0, c1, c2, 7, o1), co2 = iso_pick4(0, c1, c2, 7, o2), co3 = iso_pick4(0, c1, c2, 7, o3);
      double p1[3], p2[3], p3[3];
      double t1, t2, t3;
      if (lone_above) {
        t1 = iso_cross(qo1, qL, co1, cL, xlo, xhi, iso, p1); t2 = iso_cross(qo2, qL, co2, cL, xlo, xhi, iso, p2); t3 = iso_cross(qo3, qL, co3, cL, xlo, xhi, iso, p3);
        S.vol = S.vol + ((vtet * (1.0 - t1)) * (1.0 - t2)) * (1.0 - t3);
      } else {
        t1 = iso_cross(qL, qo1, cL, co1, xlo, xhi, iso, p1); t2 = iso_cross(qL, qo2, cL, co2, xlo, xhi, iso, p2); t3 = iso_cross(qL, qo3, cL, co3, xlo, xhi, iso, p3);
        S.vol = S.vol + (vtet - ((vtet * t1) * t2) * t3);
      }
      if (pos != lone_above) iso_tri(S, p1, p3, p2, emit); else iso_tri(S, p1, p2, p3, emit);
      ntri += 1;
    }
  }
  return ntri;
}
