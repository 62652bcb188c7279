// particles.hip -- values of cell-centred multifabs at arbitrary points of a hierarchy (vdn_sample_points) and Lagrangian tracer particles moved by Heun's method
// between the two time levels of a step (vdn_particles_*; include/varden_amd.h).  No reference counterpart (BoxLib's particle module is not used by src/); DESIGN.md
// section 21 defines the host cell, the interpolation, the face-value weights and the boundary rules, and every expression below keeps the order stated there: the
// library is built with -ffp-contract=off, so numpy float64 restates it bit for bit.
//
// Launch form.  particle_plan.h turns every level's GLOBAL box list into a map block -> box; the maps and one entry per (level, global box) -- valid box, local index,
// and, per table of a multifab list, the FV view and the face-value flags -- live on the device with the particle object, rebuilt when the layout's uid changes.
// kk_sample: one thread per particle (256-thread blocks, positions and state as separate arrays): finest covering level by one map load per level, weights, eight
// loads per component, seven lerps; components unrolled (NC) so that the move holds no scratch.  A point whose host box another rank owns gets +0.0 and ONE sum
// all-reduce per stage fills it (x + 0 + ... + 0 is x); every rank then runs the same pointwise update (kk_update): the same bits on any number of ranks.
// A move is three launches: k1 = u0(x); k2 = u1(bc(x + dt k1)), the predictor formed inside the sampling kernel; the update.  No atomics.
#include "vdn_dev.h"
#include "particle_plan.h"

namespace {
constexpr int PT_THREADS = 256, PT_MAXC = VDN_MAXCOMP;
constexpr const char *PT_MAGIC = "VDN_PARTICLES 1";

// one level of the locator (device memory, read through the constant address space)
struct PLev { double dx[3]; int lo[3], hi[3], blk[3], nb[3]; const int *map; int first; };     // first: the level's first entry in the box tables
struct PLoc { PLev lev[VDN_MAXLEV]; double len[3]; int nlev, dm; int face[3][2]; };              // len: the domain's extent; face: 0 periodic, 1 wall, 2 inlet / outlet
struct PBox { FV fv; int lo[3], hi[3]; unsigned flo[3], fhi[3]; };                              // fv.p == NULL: another rank's; flo / fhi: bit c set = component c holds a face value in that ghost layer

enum { FACE_PER = 0, FACE_WALL = 1, FACE_OPEN = 2, FACE_NONE = 3 };

// the boundary rule of one direction: returns true when p crossed an inlet / outlet face (p is then left as it is)
DEVI bool pt_boundary(double &p, double len, int flo, int fhi) {
  if (p < 0.0) {
    if (flo == FACE_OPEN) return true;
    if (flo == FACE_PER) p = p + len; else p = -p;
  } else if (p > len || (p == len && flo == FACE_PER)) {
    if (fhi == FACE_OPEN) return true;
    if (fhi == FACE_PER) p = p - len; else p = len - (p - len);
  }
  p = p < 0.0 ? 0.0 : (p > len ? len : p);      // (a NaN stays one: it has no host and samples as 0)
  return false;
}

// MODE 0: the points are (x); MODE 1: bc(x + dt k1), nothing where the predictor crosses an inlet / outlet face (the update takes k2 := k1 there)
template <int NC, int DM, int MODE>
__global__ void __launch_bounds__(PT_THREADS) kk_sample(const PLoc *Lp, const PBox *boxes, const double *__restrict__ x, const int *__restrict__ state, long n,
                                                        const double *__restrict__ k1, double dt, double *__restrict__ out, int *__restrict__ lev_out) {
  const long t = (long)blockIdx.x * PT_THREADS + threadIdx.x;
  if (t >= n) return;
  const PLoc &L = as_constant(Lp);
  double p[3] = {0.0, 0.0, 0.0};
  bool live = state == nullptr || state[t] == 0;
  #pragma unroll
  for (int d = 0; d < DM; d++) {
    p[d] = x[(long)d * n + t];
    if (MODE == 1) {
      p[d] = p[d] + dt * k1[(long)d * n + t];
      if (live && pt_boundary(p[d], L.len[d], L.face[d][0], L.face[d][1])) live = false;
    }
  }
  #pragma unroll
  for (int d = 0; d < DM; d++) live = live && p[d] >= 0.0 && p[d] <= L.len[d];
  // the finest level with a box on the point's cell
  int host = -1, box = -1;
  if (live) {
    #pragma unroll
    for (int l = VDN_MAXLEV - 1; l >= 0; l--) {
      if (l >= L.nlev || host >= 0) continue;
      const PLev &V = L.lev[l];
      int c[3];
      #pragma unroll
      for (int d = 0; d < 3; d++) {
        c[d] = V.lo[d];
        if (d < DM) { const double q = floor(p[d] / V.dx[d]); c[d] = q < (double)V.lo[d] ? V.lo[d] : (q > (double)V.hi[d] ? V.hi[d] : (int)q); }
      }
      const int b = V.map[particle_map_index(c, V.lo, V.blk, V.nb)];
      if (b >= 0) { host = l; box = V.first + b; }
    }
  }
  if (lev_out) lev_out[t] = host;
  double v[NC];
  #pragma unroll
  for (int c = 0; c < NC; c++) v[c] = 0.0;
  if (host >= 0) {
    const PBox &B = boxes[box];
    if (B.fv.p != nullptr) {
      const FV f = B.fv;
      const PLev &V = L.lev[host];
      int i[3]; double xi[3], w[3];
      #pragma unroll
      for (int d = 0; d < 3; d++) {
        i[d] = B.lo[d]; xi[d] = 0.0; w[d] = 0.0;
        if (d < DM) {
          xi[d] = p[d] / V.dx[d] - 0.5;
          const double fl = floor(xi[d]);
          w[d] = xi[d] - fl;
          i[d] = fl < (double)(B.lo[d] - 1) ? B.lo[d] - 1 : (fl > (double)B.hi[d] ? B.hi[d] : (int)fl);      // (the host cell is c or c - 1: the clamp never binds, it keeps the loads inside the fab)
        }
      }
      const long i0 = fv_idx(f, i[0], i[1], i[2]), sj = f.n0, sk = (long)f.n0 * f.n1;
      #pragma unroll
      for (int c = 0; c < NC; c++) {
        double wd[3];
        #pragma unroll
        for (int d = 0; d < DM; d++) {
          wd[d] = w[d];
          if (i[d] == B.lo[d] - 1 && ((B.flo[d] >> c) & 1u)) wd[d] = 2.0 * xi[d] + 1.0;
          if (i[d] == B.hi[d] && ((B.fhi[d] >> c) & 1u)) wd[d] = 2.0 * w[d];
        }
        const double *q = f.p + i0 + f.sc * c;
        const double a00 = q[0], b00 = q[1], a10 = q[sj], b10 = q[sj + 1];
        const double v00 = a00 + wd[0] * (b00 - a00), v10 = a10 + wd[0] * (b10 - a10);
        double r = v00 + wd[1] * (v10 - v00);
        if (DM == 3) {
          const double a01 = q[sk], b01 = q[sk + 1], a11 = q[sk + sj], b11 = q[sk + sj + 1];
          const double v01 = a01 + wd[0] * (b01 - a01), v11 = a11 + wd[0] * (b11 - a11);
          const double r1 = v01 + wd[1] * (v11 - v01);
          r = r + wd[2] * (r1 - r);
        }
        v[c] = r;
      }
    }
  }
  #pragma unroll
  for (int c = 0; c < NC; c++) out[(long)c * n + t] = v[c];
}

// x' = bc(x + (0.5 dt)(k1 + k2)); k2 := k1 where the predictor crossed an inlet / outlet face; a particle whose x' crosses one keeps its position and gets state 1
template <int DM>
__global__ void __launch_bounds__(PT_THREADS) kk_update(const PLoc *Lp, double *__restrict__ x, int *__restrict__ state, long n, const double *__restrict__ k1,
                                                        const double *__restrict__ k2, double dt, double hdt) {
  const long t = (long)blockIdx.x * PT_THREADS + threadIdx.x;
  if (t >= n) return;
  if (state[t] != 0) return;
  const PLoc &L = as_constant(Lp);
  double x0[DM], a[DM], b[DM];
  bool open = false;
  #pragma unroll
  for (int d = 0; d < DM; d++) {
    x0[d] = x[(long)d * n + t]; a[d] = k1[(long)d * n + t]; b[d] = k2[(long)d * n + t];
    double p = x0[d] + dt * a[d];
    if (pt_boundary(p, L.len[d], L.face[d][0], L.face[d][1])) open = true;
  }
  bool left = false;
  double xn[DM];
  #pragma unroll
  for (int d = 0; d < DM; d++) {
    const double kb = open ? a[d] : b[d];
    xn[d] = x0[d] + hdt * (a[d] + kb);
    if (pt_boundary(xn[d], L.len[d], L.face[d][0], L.face[d][1])) left = true;
  }
  if (left) { state[t] = 1; return; }
  #pragma unroll
  for (int d = 0; d < DM; d++) x[(long)d * n + t] = xn[d];
}

__global__ void __launch_bounds__(PT_THREADS) kk_count_active(const int *__restrict__ state, long n, double *__restrict__ out) {      // one workgroup, a fixed tree: exact (counts below 2^53)
  __shared__ double sh[PT_THREADS / 64];
  double c = 0.0;
  for (long t = threadIdx.x; t < n; t += PT_THREADS) c += state[t] == 0 ? 1.0 : 0.0;
  #pragma unroll
  for (int o = 32; o > 0; o >>= 1) c = c + __shfl_down(c, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
}   // namespace

// a table of one multifab list (components comp .. comp + nc - 1, boundary components from bccomp): kept while the multifabs' addresses and the layout stay
struct PTable { unsigned long long key = 0; PBox *d_boxes = nullptr; };
struct vdn_particles {
  long n = 0;
  int dm = 3;
  double *d_x = nullptr;             // [3][n]
  int *d_state = nullptr;            // [n]
  std::vector<double> h_x0;          // the initial positions until the first call that knows the domain has checked them
  unsigned long la_uid = 0; unsigned long long loc_key = 0;
  PLoc *d_loc = nullptr; std::vector<int *> d_maps; int nboxes = 0;
  std::vector<PTable> tables;
};

namespace {
int face_kind(int phys) {
  switch (phys) {
    case VDN_PERIODIC: return FACE_PER;
    case VDN_SLIP_WALL: case VDN_NO_SLIP_WALL: case VDN_SYMMETRY: return FACE_WALL;
    case VDN_INLET: case VDN_OUTLET: return FACE_OPEN;
    default: return FACE_NONE;
  }
}
void pt_drop_tables(vdn_particles *P) {
  for (PTable &T : P->tables) if (T.d_boxes) HIPCHK(hipFree(T.d_boxes));
  P->tables.clear();
}
void pt_drop_locator(vdn_particles *P) {
  if (ctx().inited && (P->d_loc || !P->tables.empty())) HIPCHK(hipStreamSynchronize(ctx().stream));
  pt_drop_tables(P);
  for (int *m : P->d_maps) if (m) HIPCHK(hipFree(m));
  P->d_maps.clear();
  if (P->d_loc) HIPCHK(hipFree(P->d_loc));
  P->d_loc = nullptr; P->la_uid = 0; P->loc_key = 0;
}
void pt_free(vdn_particles *P) {
  if (!P) return;
  pt_drop_locator(P);
  if (P->d_x) HIPCHK(hipFree(P->d_x));
  if (P->d_state) HIPCHK(hipFree(P->d_state));
  delete P;
}
// the checks every call on a hierarchy shares; `who` names the entry
void pt_check_hier(const char *who, int nlev, const vdn_layout *mla, const double *dx, const vdn_bc_tower *bct) {
  REQUIRE(mla, "%s: null argument (mla)", who);
  REQUIRE(nlev >= 1 && nlev <= VDN_MAXLEV, "%s: nlev = %d is outside 1 .. %d", who, nlev, VDN_MAXLEV);
  REQUIRE(nlev == mla->nlev, "%s: nlev = %d does not match the layout's %d levels", who, nlev, mla->nlev);
  REQUIRE(dx, "%s: dx is NULL (positions are physical)", who);
  REQUIRE(bct, "%s: bct is NULL (the boundary types decide face values and the boundary rule)", who);
  REQUIRE(bct->la == mla, "%s: the bc tower belongs to another layout", who);
  const int dm = ctx().prm.dm;
  REQUIRE(dm == 3 || nlev == 1, "%s: dm = 2 runs on one level (nlev = %d)", who, nlev);
  for (int n = 0; n < nlev; n++) for (int d = 0; d < dm; d++)
    REQUIRE(dx[3 * n + d] > 0.0 && dx[3 * n + d] < __builtin_huge_val(), "%s: level %d: dx[%d] = %g", who, n, d, dx[3 * n + d]);
}
void pt_check_mfs(const char *who, const char *name, int nlev, const vdn_layout *mla, vdn_multifab *const *mf, int comp, int nc) {
  REQUIRE(mf, "%s: null argument (%s)", who, name);
  REQUIRE(comp >= 0 && nc >= 1 && nc <= PT_MAXC, "%s: components %d .. %d: 1 .. %d of them, from 0 on", who, comp, comp + nc - 1, PT_MAXC);
  for (int n = 0; n < nlev; n++) {
    REQUIRE(mf[n], "%s: level %d: null multifab (%s)", who, n, name);
    REQUIRE(mf[n]->la == mla && mf[n]->lev == n, "%s: level %d: %s is not a multifab of level %d of mla", who, n, name, n);
    for (int d = 0; d < 3; d++) REQUIRE(!mf[n]->nodal[d], "%s: level %d: %s is nodal; cell-centred multifabs expected", who, n, name);
    REQUIRE(mf[n]->nc >= comp + nc, "%s: level %d: %s carries %d components, %d .. %d asked for", who, n, name, mf[n]->nc, comp, comp + nc - 1);
    REQUIRE(mf[n]->ng >= 1, "%s: level %d: %s has no ghost layer (the interpolation reads one)", who, n, name);
  }
}
// the locator of (layout, dx, boundary types): rebuilt when any of them changed
void pt_locator(vdn_particles *P, const char *who, int nlev, const vdn_layout *mla, const double *dx, const vdn_bc_tower *bct) {
  const int dm = ctx().prm.dm;
  GraphKey k; k.put(mla->uid); k.put(nlev); k.put(dm);
  for (int n = 0; n < nlev; n++) for (int d = 0; d < dm; d++) k.put(dx[3 * n + d]);
  for (int d = 0; d < 3; d++) for (int s = 0; s < 2; s++) k.put(bct->domain_bc[d][s]);
  if (P->d_loc && P->la_uid == mla->uid && P->loc_key == k.h) return;
  pt_drop_locator(P);
  PLoc L; memset(&L, 0, sizeof L);
  L.nlev = nlev; L.dm = dm;
  for (int d = 0; d < 3; d++) {
    L.len[d] = d < dm ? (double)(mla->pd[0].hi[d] - mla->pd[0].lo[d] + 1) * dx[d] : 0.0;
    for (int s = 0; s < 2; s++) {
      L.face[d][s] = d < dm ? face_kind(bct->domain_bc[d][s]) : FACE_NONE;
      REQUIRE(d >= dm || L.face[d][s] != FACE_NONE, "%s: direction %d, side %d: boundary type %d has no rule for a particle", who, d, s, bct->domain_bc[d][s]);
    }
    REQUIRE(d >= dm || mla->pd[0].lo[d] == 0, "%s: the domain's low corner must be cell 0 (prob_lo = 0)", who);
  }
  std::vector<ParticleMap> maps(nlev);
  int first = 0;
  for (int n = 0; n < nlev; n++) {
    const std::string err = particle_plan(n, mla->boxes[n], mla->pd[n], &maps[n]);
    REQUIRE(err.empty(), "%s: %s", who, err.c_str());
    PLev &V = L.lev[n];
    for (int d = 0; d < 3; d++) { V.dx[d] = d < dm ? dx[3 * n + d] : 1.0; V.lo[d] = maps[n].lo[d]; V.hi[d] = maps[n].hi[d]; V.blk[d] = maps[n].blk[d]; V.nb[d] = maps[n].n[d]; }
    V.first = first; first += (int)mla->boxes[n].size();
  }
  P->d_maps.assign(nlev, nullptr);
  for (int n = 0; n < nlev; n++) {
    const size_t bytes = sizeof(int) * maps[n].box.size();
    HIPCHK(hipMalloc((void **)&P->d_maps[n], bytes));
    HIPCHK(hipMemcpyAsync(P->d_maps[n], maps[n].box.data(), bytes, hipMemcpyHostToDevice, ctx().stream));
    L.lev[n].map = P->d_maps[n];
  }
  HIPCHK(hipMalloc((void **)&P->d_loc, sizeof(PLoc)));
  HIPCHK(hipMemcpyAsync(P->d_loc, &L, sizeof L, hipMemcpyHostToDevice, ctx().stream));
  HIPCHK(hipStreamSynchronize(ctx().stream));      // (the host arrays go out of scope)
  P->la_uid = mla->uid; P->loc_key = k.h; P->nboxes = first;
  // the initial positions, once: inside the domain
  if (!P->h_x0.empty()) {
    for (long t = 0; t < P->n; t++) for (int d = 0; d < dm; d++) {
      const double v = P->h_x0[3 * t + d];
      if (!(v >= 0.0 && v <= L.len[d])) {
        pt_drop_locator(P);
        vdn_fail("%s: particle %ld starts outside the domain (x[%d] = %.17g, the domain is 0 .. %.17g)", who, t, d, v, L.len[d]);
      }
    }
    std::vector<double>().swap(P->h_x0);
  }
}
// the box table of one multifab list (at most eight are kept: the two velocities of a step, either way round, and what a caller samples)
const PBox *pt_table(vdn_particles *P, int nlev, const vdn_layout *mla, vdn_multifab *const *mf, int comp, int nc, int bccomp, const vdn_bc_tower *bct) {
  GraphKey k; k.put(P->loc_key); k.put(comp); k.put(nc); k.put(bccomp); k.put(bct->serial);
  for (int n = 0; n < nlev; n++) { k.put(mf[n]->base); k.put(mf[n]->nc); k.put(mf[n]->ng); }
  for (PTable &T : P->tables) if (T.key == k.h) return T.d_boxes;
  if (P->tables.size() >= 8) { HIPCHK(hipStreamSynchronize(ctx().stream)); pt_drop_tables(P); }
  const int dm = ctx().prm.dm;
  std::vector<PBox> v((size_t)P->nboxes);
  size_t q = 0;
  for (int n = 0; n < nlev; n++) {
    std::vector<int> local_of(mla->boxes[n].size(), -1);
    for (int i = 0; i < (int)mla->local[n].size(); i++) local_of[mla->local[n][i]] = i;
    for (size_t g = 0; g < mla->boxes[n].size(); g++, q++) {
      PBox &B = v[q]; memset(&B, 0, sizeof B);
      const vdn_box &bx = mla->boxes[n][g];
      for (int d = 0; d < 3; d++) { B.lo[d] = bx.lo[d]; B.hi[d] = bx.hi[d]; }
      const int b = local_of[g];
      if (b < 0) continue;
      REQUIRE(b < mf[n]->nfabs(), "particles: level %d: box %d is not local", n, (int)g);
      B.fv = mf[n]->fabs[b]; B.fv.p += B.fv.sc * comp;
      for (int d = 0; d < dm; d++) for (int c = 0; c < nc; c++) {
        REQUIRE(bccomp + c < bct->ncomp_adv, "particles: boundary component %d is beyond the tower's %d", bccomp + c, bct->ncomp_adv);
        if (bx.lo[d] == mla->pd[n].lo[d] && bct->adv_bc(n, 0, d, 0, bccomp + c) == VDN_EXT_DIR) B.flo[d] |= 1u << c;
        if (bx.hi[d] == mla->pd[n].hi[d] && bct->adv_bc(n, 0, d, 1, bccomp + c) == VDN_EXT_DIR) B.fhi[d] |= 1u << c;
      }
    }
  }
  PTable T; T.key = k.h;
  HIPCHK(hipMalloc((void **)&T.d_boxes, sizeof(PBox) * v.size()));
  upload_staged(T.d_boxes, v.data(), sizeof(PBox) * v.size());
  P->tables.push_back(T);
  return T.d_boxes;
}

template <int NC, int MODE> void pt_launch_nc(int dm, const PLoc *L, const PBox *B, const double *x, const int *state, long n, const double *k1, double dt, double *out, int *lev) {
  const dim3 grid((unsigned)((n + PT_THREADS - 1) / PT_THREADS));
  if (dm == 3) hipLaunchKernelGGL((kk_sample<NC, 3, MODE>), grid, dim3(PT_THREADS), 0, ctx().stream, L, B, x, state, n, k1, dt, out, lev);
  else         hipLaunchKernelGGL((kk_sample<NC, 2, MODE>), grid, dim3(PT_THREADS), 0, ctx().stream, L, B, x, state, n, k1, dt, out, lev);
}
// one table of nc <= 4 components: every instantiation keeps its values in registers (pt_sample_all cuts wider requests into such tables)
void pt_sample(int dm, const PLoc *L, const PBox *B, int nc, const double *x, const int *state, long n, double *out, int *lev) {
  switch (nc) {
    case 1: pt_launch_nc<1, 0>(dm, L, B, x, state, n, nullptr, 0.0, out, lev); break;
    case 2: pt_launch_nc<2, 0>(dm, L, B, x, state, n, nullptr, 0.0, out, lev); break;
    case 3: pt_launch_nc<3, 0>(dm, L, B, x, state, n, nullptr, 0.0, out, lev); break;
    default: pt_launch_nc<4, 0>(dm, L, B, x, state, n, nullptr, 0.0, out, lev); break;
  }
}
// mf's components comp .. comp + nc - 1 at the positions x[3][n] -> out[nc][n] (device), every rank the full result
void pt_sample_all(vdn_particles *P, int nlev, const vdn_layout *mla, vdn_multifab *const *mf, int comp, int nc, int bccomp, const vdn_bc_tower *bct, double *d_out, int *d_lev) {
  const int dm = ctx().prm.dm;
  for (int c0 = 0; c0 < nc; c0 += 4) {
    const int m = std::min(4, nc - c0);
    const PBox *B = pt_table(P, nlev, mla, mf, comp + c0, m, bccomp + c0, bct);
    pt_sample(dm, P->d_loc, B, m, P->d_x, P->d_state, P->n, d_out + (size_t)c0 * P->n, c0 == 0 ? d_lev : nullptr);
  }
  if (comm_active()) comm_allreduce_sum_dev(d_out, (size_t)nc * P->n);
}
vdn_particles *pt_new(long n, int dm) {
  vdn_particles *P = new vdn_particles;
  P->n = n; P->dm = dm;
  try {
    HIPCHK(hipMalloc((void **)&P->d_x, sizeof(double) * 3 * (size_t)n));
    HIPCHK(hipMalloc((void **)&P->d_state, sizeof(int) * (size_t)n));
  } catch (...) { pt_free(P); throw; }
  return P;
}
// x_host[n][3] -> d_x[3][n]
void pt_upload_positions(vdn_particles *P, const double *x_host) {
  std::vector<double> soa(3 * (size_t)P->n);
  for (long t = 0; t < P->n; t++) for (int d = 0; d < 3; d++) soa[(size_t)d * P->n + t] = d < P->dm ? x_host[3 * t + d] : 0.0;
  HIPCHK(hipMemcpyAsync(P->d_x, soa.data(), sizeof(double) * soa.size(), hipMemcpyHostToDevice, ctx().stream));
  HIPCHK(hipStreamSynchronize(ctx().stream));
}
}   // namespace

extern "C" int vdn_particles_create(long n, const double *x_host, vdn_particles **out) {
  VDN_TRY
  REQUIRE(ctx().inited, "vdn_particles_create: vdn_init has not been called");
  REQUIRE(x_host && out, "vdn_particles_create: null argument (x_host, P)");
  REQUIRE(n >= 1, "vdn_particles_create: n = %ld particles (at least 1)", n);
  const int dm = ctx().prm.dm;
  for (long t = 0; t < n; t++) for (int d = 0; d < dm; d++)
    REQUIRE(fabs(x_host[3 * t + d]) < __builtin_huge_val(), "vdn_particles_create: particle %ld: x[%d] is not finite", t, d);
  vdn_particles *P = pt_new(n, dm);
  try {
    pt_upload_positions(P, x_host);
    HIPCHK(hipMemsetAsync(P->d_state, 0, sizeof(int) * (size_t)n, ctx().stream));
    P->h_x0.assign(x_host, x_host + 3 * (size_t)n);
  } catch (...) { pt_free(P); throw; }
  *out = P;
  VDN_CATCH
}

extern "C" int vdn_particles_destroy(vdn_particles *P) {
  VDN_TRY
  pt_free(P);
  VDN_CATCH
}

extern "C" int vdn_particles_count(vdn_particles *P, long *n, long *active) {
  VDN_TRY
  REQUIRE(ctx().inited, "vdn_particles_count: vdn_init has not been called");
  REQUIRE(P, "vdn_particles_count: null argument (P)");
  if (n) *n = P->n;
  if (active) {
    hipLaunchKernelGGL(kk_count_active, dim3(1), dim3(PT_THREADS), 0, ctx().stream, (const int *)P->d_state, P->n, ctx().d_scal);
    *active = (long)read_scalar1(ctx().d_scal);
  }
  VDN_CATCH
}

extern "C" int vdn_particles_get(vdn_particles *P, double *x_host, int *state_host) {
  VDN_TRY
  REQUIRE(ctx().inited, "vdn_particles_get: vdn_init has not been called");
  REQUIRE(P, "vdn_particles_get: null argument (P)");
  if (x_host) {
    std::vector<double> soa(3 * (size_t)P->n);
    HIPCHK(hipMemcpyAsync(soa.data(), P->d_x, sizeof(double) * soa.size(), hipMemcpyDeviceToHost, ctx().stream));
    HIPCHK(hipStreamSynchronize(ctx().stream));
    for (long t = 0; t < P->n; t++) for (int d = 0; d < 3; d++) x_host[3 * t + d] = soa[(size_t)d * P->n + t];
  }
  if (state_host) {
    HIPCHK(hipMemcpyAsync(state_host, P->d_state, sizeof(int) * (size_t)P->n, hipMemcpyDeviceToHost, ctx().stream));
    HIPCHK(hipStreamSynchronize(ctx().stream));
  }
  VDN_CATCH
}

extern "C" int vdn_particles_advance(vdn_particles *P, int nlev, vdn_layout *mla, vdn_multifab *const *u0, vdn_multifab *const *u1, const double *dx,
                                     const vdn_bc_tower *bct, double dt) {
  VDN_TRY
  const char *who = "vdn_particles_advance";
  REQUIRE(ctx().inited, "%s: vdn_init has not been called", who);
  REQUIRE(P, "%s: null argument (P)", who);
  pt_check_hier(who, nlev, mla, dx, bct);
  const int dm = ctx().prm.dm;
  REQUIRE(P->dm == dm, "%s: the particles were created for dm = %d", who, P->dm);
  pt_check_mfs(who, "u0", nlev, mla, u0, 0, dm);
  pt_check_mfs(who, "u1", nlev, mla, u1, 0, dm);
  REQUIRE(fabs(dt) < __builtin_huge_val(), "%s: dt is not finite", who);
  pt_locator(P, who, nlev, mla, dx, bct);
  const PBox *B0 = pt_table(P, nlev, mla, u0, 0, dm, 0, bct);
  const PBox *B1 = pt_table(P, nlev, mla, u1, 0, dm, 0, bct);
  B0 = pt_table(P, nlev, mla, u0, 0, dm, 0, bct);      // (the second table may have emptied a full cache)
  ArenaScope arena;
  const long n = P->n;
  double *k1 = (double *)arena_alloc(sizeof(double) * 3 * (size_t)n), *k2 = (double *)arena_alloc(sizeof(double) * 3 * (size_t)n);
  const bool ranks = comm_active();
  const dim3 grid((unsigned)((n + PT_THREADS - 1) / PT_THREADS));
  hipStream_t st = ctx().stream;
  if (dm == 3) {
    pt_launch_nc<3, 0>(3, P->d_loc, B0, P->d_x, P->d_state, n, nullptr, 0.0, k1, nullptr);
    if (ranks) comm_allreduce_sum_dev(k1, 3 * (size_t)n);
    pt_launch_nc<3, 1>(3, P->d_loc, B1, P->d_x, P->d_state, n, k1, dt, k2, nullptr);
    if (ranks) comm_allreduce_sum_dev(k2, 3 * (size_t)n);
    hipLaunchKernelGGL((kk_update<3>), grid, dim3(PT_THREADS), 0, st, (const PLoc *)P->d_loc, P->d_x, P->d_state, n, (const double *)k1, (const double *)k2, dt, 0.5 * dt);
  } else {
    pt_launch_nc<2, 0>(2, P->d_loc, B0, P->d_x, P->d_state, n, nullptr, 0.0, k1, nullptr);
    if (ranks) comm_allreduce_sum_dev(k1, 2 * (size_t)n);
    pt_launch_nc<2, 1>(2, P->d_loc, B1, P->d_x, P->d_state, n, k1, dt, k2, nullptr);
    if (ranks) comm_allreduce_sum_dev(k2, 2 * (size_t)n);
    hipLaunchKernelGGL((kk_update<2>), grid, dim3(PT_THREADS), 0, st, (const PLoc *)P->d_loc, P->d_x, P->d_state, n, (const double *)k1, (const double *)k2, dt, 0.5 * dt);
  }
  arena.release();
  VDN_CATCH
}

// shared by vdn_particles_sample and vdn_sample_points: val_host[n][nc], lev_host[n] (may be NULL)
static void pt_sample_to_host(vdn_particles *P, const char *who, int nlev, vdn_layout *mla, vdn_multifab *const *mf, int comp, int nc, int bccomp, const double *dx,
                              const vdn_bc_tower *bct, double *val_host, int *lev_host) {
  pt_check_hier(who, nlev, mla, dx, bct);
  pt_check_mfs(who, "mf", nlev, mla, mf, comp, nc);
  REQUIRE(bccomp >= 0 && bccomp + nc <= bct->ncomp_adv, "%s: boundary components %d .. %d, the tower holds %d", who, bccomp, bccomp + nc - 1, bct->ncomp_adv);
  REQUIRE(val_host, "%s: null argument (val_host)", who);
  pt_locator(P, who, nlev, mla, dx, bct);
  ArenaScope arena;
  const long n = P->n;
  double *d_out = (double *)arena_alloc(sizeof(double) * (size_t)nc * n);
  int *d_lev = (int *)arena_alloc(sizeof(int) * (size_t)n);
  pt_sample_all(P, nlev, mla, mf, comp, nc, bccomp, bct, d_out, d_lev);
  std::vector<double> soa((size_t)nc * n);
  HIPCHK(hipMemcpyAsync(soa.data(), d_out, sizeof(double) * soa.size(), hipMemcpyDeviceToHost, ctx().stream));
  if (lev_host) HIPCHK(hipMemcpyAsync(lev_host, d_lev, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, ctx().stream));
  HIPCHK(hipStreamSynchronize(ctx().stream));
  for (long t = 0; t < n; t++) for (int c = 0; c < nc; c++) val_host[(size_t)t * nc + c] = soa[(size_t)c * n + t];
  arena.release();
}

extern "C" int vdn_particles_sample(vdn_particles *P, int nlev, vdn_layout *mla, vdn_multifab *const *mf, int comp, int nc, int bccomp, const double *dx,
                                    const vdn_bc_tower *bct, double *val_host, int *lev_host) {
  VDN_TRY
  REQUIRE(ctx().inited, "vdn_particles_sample: vdn_init has not been called");
  REQUIRE(P, "vdn_particles_sample: null argument (P)");
  REQUIRE(P->dm == ctx().prm.dm, "vdn_particles_sample: the particles were created for dm = %d", P->dm);
  pt_sample_to_host(P, "vdn_particles_sample", nlev, mla, mf, comp, nc, bccomp, dx, bct, val_host, lev_host);
  VDN_CATCH
}

extern "C" int vdn_sample_points(int nlev, vdn_layout *mla, vdn_multifab *const *mf, int comp, int nc, int bccomp, const double *dx, const vdn_bc_tower *bct,
                                 long n, const double *x_host, double *val_host, int *lev_host) {
  VDN_TRY
  REQUIRE(ctx().inited, "vdn_sample_points: vdn_init has not been called");
  REQUIRE(x_host, "vdn_sample_points: null argument (x_host)");
  REQUIRE(n >= 1, "vdn_sample_points: n = %ld points (at least 1)", n);
  vdn_particles *P = pt_new(n, ctx().prm.dm);      // a particle set for the length of the call; positions outside the domain (or not finite) have no host: level -1, value 0
  try {
    pt_upload_positions(P, x_host);
    HIPCHK(hipMemsetAsync(P->d_state, 0, sizeof(int) * (size_t)n, ctx().stream));
    pt_sample_to_host(P, "vdn_sample_points", nlev, mla, mf, comp, nc, bccomp, dx, bct, val_host, lev_host);
  } catch (...) { pt_free(P); throw; }
  pt_free(P);
  VDN_CATCH
}

// ---- particle files: a text header, then little-endian state (int32[n]), positions (float64[n][3]) and columns (float64[ncol][n]) ---------------------------------
extern "C" int vdn_particles_write(vdn_particles *P, const char *path, double time, int ncol, const char *const *names, const double *cols) {
  VDN_TRY
  REQUIRE(ctx().inited, "vdn_particles_write: vdn_init has not been called");
  REQUIRE(P && path, "vdn_particles_write: null argument (P, path)");
  REQUIRE(ncol >= 0 && (ncol == 0 || (names && cols)), "vdn_particles_write: %d columns need names and values", ncol);
  for (int c = 0; c < ncol; c++) REQUIRE(names[c] && names[c][0] && !strpbrk(names[c], " \t\r\n"), "vdn_particles_write: column %d: a name is one word", c);
  const size_t n = (size_t)P->n;
  std::vector<double> x(3 * n); std::vector<int> state(n);
  REQUIRE(vdn_particles_get(P, x.data(), state.data()) == 0, "vdn_particles_write: %s", vdn_last_error());
  if (ctx().rank != 0) return 0;                 // every rank holds the same particles: rank 0 writes
  FILE *f = fopen(path, "wb");
  REQUIRE(f, "vdn_particles_write: cannot open %s", path);
  fprintf(f, "%s\ndm %d\nn %ld\nncol %d\n", PT_MAGIC, P->dm, P->n, ncol);
  for (int c = 0; c < ncol; c++) fprintf(f, "%s\n", names[c]);
  fprintf(f, "time %.17g\n", time);
  bool ok = fwrite(state.data(), sizeof(int), n, f) == n && fwrite(x.data(), sizeof(double), 3 * n, f) == 3 * n;
  if (ncol > 0) ok = ok && fwrite(cols, sizeof(double), (size_t)ncol * n, f) == (size_t)ncol * n;
  ok = (fclose(f) == 0) && ok;
  REQUIRE(ok, "vdn_particles_write: writing %s failed", path);
  VDN_CATCH
}

extern "C" int vdn_particles_read(const char *path, vdn_particles **out, double *time) {
  VDN_TRY
  REQUIRE(ctx().inited, "vdn_particles_read: vdn_init has not been called");
  REQUIRE(path && out, "vdn_particles_read: null argument (path, P)");
  FILE *f = fopen(path, "rb");
  REQUIRE(f, "vdn_particles_read: cannot open %s", path);
  struct Closer { FILE *f; ~Closer() { if (f) fclose(f); } } closer{ f };
  char line[512];
  REQUIRE(fgets(line, sizeof line, f) && strncmp(line, PT_MAGIC, strlen(PT_MAGIC)) == 0 && line[strlen(PT_MAGIC)] == '\n',
          "vdn_particles_read: %s is not a particle file (its first line is not \"%s\")", path, PT_MAGIC);
  int dm = 0, ncol = -1; long n = 0; double t = 0.0;
  REQUIRE(fgets(line, sizeof line, f) && sscanf(line, "dm %d", &dm) == 1 && fgets(line, sizeof line, f) && sscanf(line, "n %ld", &n) == 1 &&
          fgets(line, sizeof line, f) && sscanf(line, "ncol %d", &ncol) == 1, "vdn_particles_read: %s: the header is short", path);
  REQUIRE((dm == 2 || dm == 3) && n >= 1 && ncol >= 0 && ncol <= 4096, "vdn_particles_read: %s: dm = %d, n = %ld, ncol = %d", path, dm, n, ncol);
  REQUIRE(dm == ctx().prm.dm, "vdn_particles_read: %s holds dm = %d particles, the run is dm = %d", path, dm, ctx().prm.dm);
  for (int c = 0; c < ncol; c++) REQUIRE(fgets(line, sizeof line, f) != nullptr, "vdn_particles_read: %s: the header is short", path);
  REQUIRE(fgets(line, sizeof line, f) && strncmp(line, "time ", 5) == 0, "vdn_particles_read: %s: the header is short", path);
  t = strtod(line + 5, nullptr);
  std::vector<int> state((size_t)n); std::vector<double> x(3 * (size_t)n);
  REQUIRE(fread(state.data(), sizeof(int), (size_t)n, f) == (size_t)n && fread(x.data(), sizeof(double), 3 * (size_t)n, f) == 3 * (size_t)n,
          "vdn_particles_read: %s is short: it ends inside the state or the positions of its %ld particles", path, n);
  if (ncol > 0) {
    const long here = ftell(f);
    REQUIRE(fseek(f, 0, SEEK_END) == 0 && ftell(f) - here >= (long)(sizeof(double) * (size_t)ncol * (size_t)n), "vdn_particles_read: %s is short: it ends inside its %d columns", path, ncol);
  }
  vdn_particles *P = pt_new(n, dm);
  try {
    pt_upload_positions(P, x.data());
    HIPCHK(hipMemcpyAsync(P->d_state, state.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, ctx().stream));
    HIPCHK(hipStreamSynchronize(ctx().stream));
  } catch (...) { pt_free(P); throw; }
  *out = P;
  if (time) *time = t;
  VDN_CATCH
}
