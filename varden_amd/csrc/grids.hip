// grids.hip -- the grid generation that sits in front of the AMR hot path: tag_boxes (src/tag_boxes.f90:17-216) on the device and
// FBoxLib's make_new_grids (src/initialize.f90:247-248, src/regrid.f90:148-149): the per-cell maps on the device, the clustering of the block lattice
// (1/blocking^3 of the cells) on the host.
//
// make_new_grids is not in the reference tree (FBoxLib); the call sites and the probin parameters fix what goes in and out, the
// procedure below is ours:
//   1. tags = tag_boxes(first component of `s`, level) on the valid cells of the level (the reference's thresholds);
//   2. the tags are grown by amr_buf_width cells (probin.template:147-154) and clipped to the nesting region: the cells of the
//      level that keep `nest` cells of the level between themselves and any cell outside it (domain boundaries do not count; a periodic face is no boundary: the maps wrap) --
//      the coarse-fine interpolation of the finer level then always finds its parents on this level;
//   3. Berger-Rigoutsos clustering on the lattice of cluster_blocking_factor^3 blocks: take the bounding box of the tagged
//      blocks; accept it when tagged/total >= cluster_min_eff or it cannot be cut; otherwise cut it at a hole of the tag
//      signature, else at the strongest inflection of the signature's second difference, else in the middle of the longest side,
//      and recurse;
//   4. the boxes are refined by ref_ratio and chopped to max_grid_size.
// Output: boxes of level+1 in its own index space, disjoint, every tagged cell covered, blocking-factor aligned.
// Step 1 has a second form, chosen at run time (vdn_tag_boxes_by / vdn_make_new_grids_by): up to 8 criteria over a scalar, its undivided gradient, the
// vorticity or the velocity magnitude, ORed per cell in one pass (kk_tag_by); steps 2-4 are shared (new_grids_from_tags).
#include "vdn_dev.h"
#include "derived.h"
#include "cluster.h"
#include <vector>
#include <algorithm>

__global__ void kk_tag(FV s, unsigned char *tags, int n0, int n1, int d0, int d1, int d2, int rule, double tlo, double thi, Range3 r) {
  THREAD_IJK(r)
  if (!in_range) return;
  const double v = fv_get(s, i, j, k);
  const bool t = rule == 0 ? (v > tlo) : (v > tlo && v < thi);
  tags[(size_t)(i - d0) + (size_t)n0 * ((size_t)(j - d1) + (size_t)n1 * (size_t)(k - d2))] = t ? 1 : 0;
}

// ---- tagging by criteria ---------------------------------------------------------------------------------------------------------------------------
// A cell is tagged when gt < value < lt holds for ANY row of the table (both strict, as in tag_boxes.f90; a NaN value fails both comparisons).  The table
// travels by value in the kernel arguments (200 bytes).  MASK says at compile time which kinds of field the table holds, so a rule set reads only what it
// needs: scalars alone touch neither u nor the neighbours of s -- 8 B read and 1 B written per cell, kk_tag's traffic; the vorticity reads the three
// components of u once each (their neighbours are the same cache lines one row or plane on): 24 B per cell.  Nothing derived is stored: at 512^3 a
// vorticity multifab would be 1 GB written and read back.  Streaming, no LDS, no atomics; x fastest, 64 x 4, as kk_tag.
struct TagRule { int field, comp; double gt, lt; };
struct TagTable { int n, pad; TagRule r[VDN_TAG_MAX_CRITERIA]; };
enum { TAG_HAS_SCALAR = 1 << VDN_TAG_SCALAR, TAG_HAS_GRAD = 1 << VDN_TAG_SCALAR_GRAD, TAG_HAS_VORT = 1 << VDN_TAG_VORTICITY, TAG_HAS_MAGVEL = 1 << VDN_TAG_MAGVEL };
DEVI double tag_max(double a, double b) { return (a >= b || a != a) ? a : b; }       // a NaN operand stays (fmax would drop it)
// max(|s(i+e_D) - s(i)|, |s(i) - s(i-e_D)|), undivided
template <int D> DEVI double tag_grad(const FV &s, int c, int i, int j, int k) {
  const double s0 = fv_get(s, i, j, k, c);
  return tag_max(fabs(fv_get(s, i + (D == 0), j + (D == 1), k + (D == 2), c) - s0), fabs(s0 - fv_get(s, i - (D == 0), j - (D == 1), k - (D == 2), c)));
}
template <int MASK>
__global__ void __launch_bounds__(256) kk_tag_by(FV s, FV u, VortArgs A, TagTable T, unsigned char *tags, int n0, int n1, int d0, int d1, int d2, Range3 r) {
  THREAD_IJK(r)
  if (!in_range) return;
  double vort = 0.0, mag = 0.0;
  if (MASK & TAG_HAS_VORT) { vort = vort_value(u, A, i, j, k); if (A.dm == 2) vort = fabs(vort); }
  if (MASK & TAG_HAS_MAGVEL) mag = magvel_value(u, A.dm, i, j, k);
  bool t = false;
  #pragma unroll
  for (int q = 0; q < VDN_TAG_MAX_CRITERIA; q++) {
    if (q >= T.n) break;
    const int f = T.r[q].field, c = T.r[q].comp;
    double v = mag;
    if ((MASK & TAG_HAS_SCALAR) && f == VDN_TAG_SCALAR) v = fv_get(s, i, j, k, c);
    else if ((MASK & TAG_HAS_GRAD) && f == VDN_TAG_SCALAR_GRAD) {
      v = tag_max(tag_grad<0>(s, c, i, j, k), tag_grad<1>(s, c, i, j, k));
      if (A.dm == 3) v = tag_max(v, tag_grad<2>(s, c, i, j, k));
    } else if ((MASK & TAG_HAS_VORT) && f == VDN_TAG_VORTICITY) v = vort;
    t = t || (v > T.r[q].gt && v < T.r[q].lt);
  }
  tags[(size_t)(i - d0) + (size_t)n0 * ((size_t)(j - d1) + (size_t)n1 * (size_t)(k - d2))] = t ? 1 : 0;
}
template <int MASK> static void launch_tag_by(const Range3 &r, FV s, FV u, const VortArgs &A, const TagTable &T, unsigned char *tags, const int *n, const vdn_box &pd) {
  hipLaunchKernelGGL((kk_tag_by<MASK>), grid_for(r), dim3(64, 4, 1), 0, ctx().stream, s, u, A, T, tags, n[0], n[1], pd.lo[0], pd.lo[1], pd.lo[2], r);
}

// the byte maps of make_new_grids on the device: one byte per cell of the level's domain, x fastest
__global__ void kk_count_bytes(const unsigned char *a, size_t n, unsigned long long *out) {
  unsigned long long c = 0;
  for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < n; q += (size_t)gridDim.x * blockDim.x) c += a[q];
  for (int o = 32; o > 0; o >>= 1) c += __shfl_down(c, o);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}
__global__ void kk_fill_bytes(unsigned char *a, int n0, int n1, Range3 r) {
  THREAD_IJK(r)
  if (in_range) a[(size_t)i + (size_t)n0 * ((size_t)j + (size_t)n1 * (size_t)k)] = 1;
}
// box dilation (OR) or erosion (AND) by `width` cells in direction d; cells outside the domain do not take part, except across a periodic face, where the
// map wraps (a refined box at a periodic face needs its parents' periodic images underneath it: without the wrap the nesting region ignored them and
// inputs_RayleighTaylor_2d met an improperly nested level at its 31st regrid)
__global__ void kk_sweep_bytes(const unsigned char *in, unsigned char *out, int n0, int n1, int n2, int d, int width, int dilate, int periodic) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x), j = (int)(blockIdx.y * blockDim.y + threadIdx.y), k = (int)(blockIdx.z * blockDim.z + threadIdx.z);
  if (i >= n0 || j >= n1 || k >= n2) return;
  const size_t c = (size_t)i + (size_t)n0 * ((size_t)j + (size_t)n1 * (size_t)k);
  const size_t stride = d == 0 ? 1 : (d == 1 ? (size_t)n0 : (size_t)n0 * n1);
  const int q = d == 0 ? i : (d == 1 ? j : k), nq = d == 0 ? n0 : (d == 1 ? n1 : n2);
  unsigned char v = dilate ? 0 : 1;
  for (int w = -width; w <= width; w++) {
    int ww = w;
    if (q + w < 0 || q + w >= nq) { if (!periodic) continue; ww = ((q + w) % nq + nq) % nq - q; }
    const unsigned char x = in[(long)c + (long)ww * (long)stride];
    if (dilate) v |= x; else v &= x;
  }
  out[c] = v;
}
// per block of blocking^dm cells: ok = every cell inside the nesting region, t = ok and any cell tagged
__global__ void kk_block_lattice(const unsigned char *tags, const unsigned char *inside, unsigned char *t, unsigned char *ok, int n0, int n1, int g0, int g1,
                                 int blocking, int bz, Range3 r) {
  THREAD_IJK(r)
  if (!in_range) return;
  bool any = false, all_in = true;
  for (int c = 0; c < bz; c++) for (int b = 0; b < blocking; b++) for (int a = 0; a < blocking; a++) {
    const size_t q = (size_t)(i * blocking + a) + (size_t)n0 * ((size_t)(j * blocking + b) + (size_t)n1 * (size_t)(k * bz + c));
    any = any || tags[q]; all_in = all_in && inside[q];
  }
  t[(size_t)i + (size_t)g0 * ((size_t)j + (size_t)g1 * (size_t)k)] = (any && all_in) ? 1 : 0;
  ok[(size_t)i + (size_t)g0 * ((size_t)j + (size_t)g1 * (size_t)k)] = all_in ? 1 : 0;
}

using namespace vdn_cluster;

// tag_boxes (src/tag_boxes.f90:17-39 driver, 41-127 2-D, 128-216 3-D) of one level: a byte per cell of the level's DOMAIN (x fastest), 1 where
// the first component of s exceeds the level's threshold; cells outside the level's boxes stay 0; all ranks end with the same bitmap.
// Fills `tags` (freed with its owner).
// a device buffer that goes with its scope: a throwing HIPCHK between hipMalloc and hipFree leaked the four buffers of make_new_grids
template <class T> struct DevBuf {
  T *p = nullptr;
  DevBuf() {}
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { if (p) (void)hipFree(p); }
  void alloc(size_t count) { HIPCHK(hipMalloc((void **)&p, count * sizeof(T))); }
};
typedef DevBuf<unsigned char> DevBytes;
static size_t level_cells(const vdn_multifab *s, int n[3]) {
  const vdn_box &pd = s->la->pd[s->lev];
  for (int d = 0; d < 3; d++) n[d] = pd.hi[d] - pd.lo[d] + 1;
  return (size_t)n[0] * n[1] * n[2];
}
static void tag_level(const vdn_multifab *s, int lev1, DevBytes &tags) {
  const vdn_box &pd = s->la->pd[s->lev];
  int n[3]; for (int d = 0; d < 3; d++) n[d] = pd.hi[d] - pd.lo[d] + 1;
  const int pt = ctx().prm.prob_type;
  REQUIRE(pt == 1 || pt == 2 || pt == 3, "tag_boxes: unsupported prob_type %d (tag_boxes.f90:212)", pt);
  int rule = 0; double tlo = 0.0, thi = 0.0;
  if (pt == 3) { rule = 1; tlo = 1.2; thi = 1.8; } else { tlo = lev1 == 1 ? 1.01 : (lev1 == 2 ? 1.1 : 1.5); }
  const size_t ncell = (size_t)n[0] * n[1] * n[2];
  tags.alloc(ncell);
  unsigned char *d_tags = tags.p;
  HIPCHK(hipMemsetAsync(d_tags, 0, ncell, ctx().stream));
  for (int b = 0; b < s->nfabs(); b++) {
    Range3 r; for (int d = 0; d < 3; d++) { r.lo[d] = s->vbox[b].lo[d]; r.hi[d] = s->vbox[b].hi[d]; }
    hipLaunchKernelGGL(kk_tag, grid_for(r), dim3(64, 4, 1), 0, ctx().stream, s->fabs[b], d_tags, n[0], n[1], pd.lo[0], pd.lo[1], pd.lo[2], rule, tlo, thi, r);
  }
  comm_allreduce_max_u8_dev(d_tags, ncell);                // the tags of the other ranks' boxes: every rank sees the same bitmap
}
// the same bitmap from criteria chosen at run time (include/varden_amd.h: vdn_tag_criterion): one launch of kk_tag_by per local box evaluates every
// criterion.  Velocity criteria fill the ghost cells of u the way make_vorticity / make_magvel do (same-level fill, then physbc for the vorticity); the
// gradient reads one ghost layer of s as the caller left it.  `who` names the entry point in the messages.
static void tag_level_by(const char *who, const vdn_multifab *s, vdn_multifab *u, const double *dx, const vdn_bc_tower *bct, int lev1,
                         int ncrit, const vdn_tag_criterion *crit, DevBytes &tags) {
  REQUIRE(s && crit, "%s: null argument", who);
  REQUIRE(ncrit >= 1 && ncrit <= VDN_TAG_MAX_CRITERIA, "%s: %d criteria (1 .. %d)", who, ncrit, VDN_TAG_MAX_CRITERIA);
  REQUIRE(lev1 >= 1 && lev1 <= VDN_MAXLEV, "%s: level %d (1 .. %d)", who, lev1, VDN_MAXLEV);
  const int dm = ctx().prm.dm;
  TagTable T; T.n = ncrit; T.pad = 0;
  int mask = 0;
  for (int q = 0; q < VDN_TAG_MAX_CRITERIA; q++) {
    TagRule &r = T.r[q]; r.field = VDN_TAG_SCALAR; r.comp = 0; r.gt = __builtin_huge_val(); r.lt = -__builtin_huge_val();
    if (q >= ncrit) continue;
    const vdn_tag_criterion &c = crit[q];
    REQUIRE(c.field >= VDN_TAG_SCALAR && c.field <= VDN_TAG_MAGVEL, "%s: criterion %d: unknown field %d", who, q, c.field);
    if (c.field == VDN_TAG_SCALAR || c.field == VDN_TAG_SCALAR_GRAD) {
      REQUIRE(c.comp >= 0 && c.comp < s->nc, "%s: criterion %d: component %d of a multifab with %d", who, q, c.comp, s->nc);
      REQUIRE(c.field == VDN_TAG_SCALAR || s->ng >= 1, "%s: criterion %d: a gradient criterion reads one ghost cell, the state has none", who, q);
      r.comp = c.comp;
    } else {
      REQUIRE(u, "%s: criterion %d reads the velocity: u is null", who, q);
      REQUIRE(u->la == s->la && u->lev == s->lev && u->nfabs() == s->nfabs() && u->nc >= dm, "%s: u and s differ in level or boxes, or u has fewer than %d components", who, dm);
      if (c.field == VDN_TAG_VORTICITY) REQUIRE(dx && bct && u->ng >= 1, "%s: criterion %d: the vorticity needs dx, the bc tower and one ghost cell of u", who, q);
    }
    r.field = c.field; r.gt = c.gt[lev1 - 1]; r.lt = c.lt[lev1 - 1];
    mask |= 1 << c.field;
  }
  if (mask & TAG_HAS_VORT) { mf_fill_boundary(u); mf_physbc(u, 0, 0, dm, bct, false); }     // k_make_vorticity's fills
  else if (mask & TAG_HAS_MAGVEL) mf_fill_boundary(u);                                        // k_make_magvel's
  const vdn_box &pd = s->la->pd[s->lev];
  int n[3]; const size_t ncell = level_cells(s, n);
  tags.alloc(ncell);
  HIPCHK(hipMemsetAsync(tags.p, 0, ncell, ctx().stream));
  for (int b = 0; b < s->nfabs(); b++) {
    Range3 r; for (int d = 0; d < 3; d++) { r.lo[d] = s->vbox[b].lo[d]; r.hi[d] = s->vbox[b].hi[d]; }
    VortArgs A = VortArgs(); A.dm = dm;
    if (mask & TAG_HAS_VORT) A = vort_args(u, b, bct, dx, dm, 0);
    const FV fu = (mask & (TAG_HAS_VORT | TAG_HAS_MAGVEL)) ? u->fabs[b] : FV();
    switch (mask) {
#define TAG_CASE(M) case M: launch_tag_by<M>(r, s->fabs[b], fu, A, T, tags.p, n, pd); break;
      TAG_CASE(1) TAG_CASE(2) TAG_CASE(3) TAG_CASE(4) TAG_CASE(5) TAG_CASE(6) TAG_CASE(7) TAG_CASE(8)
      TAG_CASE(9) TAG_CASE(10) TAG_CASE(11) TAG_CASE(12) TAG_CASE(13) TAG_CASE(14) TAG_CASE(15)
#undef TAG_CASE
      default: vdn_fail("%s: no criterion", who);
    }
  }
  comm_allreduce_max_u8_dev(tags.p, ncell);
}
static void tags_to_host(const vdn_multifab *s, const DevBytes &tags, unsigned char *tags_host) {
  int n[3]; const size_t ncell = level_cells(s, n);
  HIPCHK(hipMemcpyAsync(tags_host, tags.p, ncell, hipMemcpyDeviceToHost, ctx().stream));
  HIPCHK(hipStreamSynchronize(ctx().stream));
}
// the tag bitmap alone (the parity test against the restated tag_boxes_3d): tags_host holds one byte per cell of the level's domain
extern "C" int vdn_tag_boxes(const vdn_multifab *s, int lev1, unsigned char *tags_host) {
  VDN_TRY
  REQUIRE(s && tags_host, "vdn_tag_boxes: null argument");
  DevBytes tags;
  tag_level(s, lev1, tags);
  tags_to_host(s, tags, tags_host);
  VDN_CATCH
}
extern "C" int vdn_tag_boxes_by(const vdn_multifab *s, vdn_multifab *u, const double *dx, const vdn_bc_tower *bct, int lev1,
                                int ncrit, const vdn_tag_criterion *crit, unsigned char *tags_host) {
  VDN_TRY
  REQUIRE(ctx().inited, "vdn_init has not been called");
  REQUIRE(s && tags_host, "vdn_tag_boxes_by: null argument");
  DevBytes tags;
  tag_level_by("vdn_tag_boxes_by", s, u, dx, bct, lev1, ncrit, crit, tags);
  tags_to_host(s, tags, tags_host);
  VDN_CATCH
}

// what make_new_grids checks before it tags
static void check_grid_args(const char *who, const vdn_multifab *s, int min_width, int blocking, int max_grid_size, const vdn_box *boxes_out, const int *nboxes_out) {
  REQUIRE(s && boxes_out && nboxes_out, "%s: null argument", who);
  REQUIRE(blocking >= 1 && min_width >= 1 && max_grid_size >= 2 * blocking, "%s: bad clustering parameters", who);
  int n[3]; level_cells(s, n);
  const int dm = ctx().prm.dm;
  for (int d = 0; d < dm; d++) REQUIRE(n[d] % blocking == 0, "%s: the domain extent %d is not a multiple of the blocking factor %d", who, n[d], blocking);
}
// steps 2-4 of make_new_grids from a tag bitmap of the level of `s` (one byte per cell of its domain, the same on every rank): the boxes of the next finer
// level in ITS index space.  The bitmap is grown in place.
static void new_grids_from_tags(const char *who, const vdn_multifab *s, DevBytes &tags, int buf_wid, int nest, double min_eff, int min_width, int blocking,
                                int max_grid_size, int maxboxes, vdn_box *boxes_out, int *nboxes_out, long *ntagged) {
  const vdn_layout *la = s->la;
  const vdn_box &pd = la->pd[s->lev];
  int n[3]; const size_t ncell = level_cells(s, n);
  const int dm = ctx().prm.dm;
  Lattice G; for (int d = 0; d < 3; d++) G.n[d] = d < dm ? n[d] / blocking : 1;
  *nboxes_out = 0;
  {
  // 2. on the device (a 512^3 level is 134 M cells: the host loops of rounds 2-5 took 5 s of a 0.5 s step, tools/probes/regrid_profile_probe.py): count the tags,
  // grow them by buf_wid (box dilation, one direction after the other), inside[] = 1 on the cells of the level -- every box, on any rank --, shrunk by `nest`
  // the same way (cells outside the domain count as inside: a level may touch the domain boundary)
  hipStream_t st = ctx().stream;
  DevBytes in, tmp; DevBuf<unsigned long long> cnt;                  // with `tags`: the four device buffers, freed at the end of this block, thrown or not
  in.alloc(ncell); tmp.alloc(ncell); cnt.alloc(1);
  unsigned char *&d_tags = tags.p, *&d_in = in.p, *&d_tmp = tmp.p; unsigned long long *d_cnt = cnt.p;
  HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(kk_count_bytes, dim3((unsigned)std::min<size_t>((ncell + 255) / 256, 4096)), dim3(256), 0, st, d_tags, ncell, d_cnt);
  unsigned long long nt = 0;
  HIPCHK(hipMemcpyAsync(&nt, d_cnt, sizeof(nt), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (ntagged) *ntagged = (long)nt;
  if (nt == 0) return;
  Range3 whole_cells; for (int d = 0; d < 3; d++) { whole_cells.lo[d] = 0; whole_cells.hi[d] = n[d] - 1; }
  auto sweep = [&](unsigned char *&a, unsigned char *&tmp, int width, int dilate) {
    if (width <= 0) return;
    for (int d = 0; d < dm; d++) {
      hipLaunchKernelGGL(kk_sweep_bytes, grid_for(whole_cells), dim3(64, 4, 1), 0, st, (const unsigned char *)a, tmp, n[0], n[1], n[2], d, width, dilate, la->pmask[d] ? 1 : 0);
      std::swap(a, tmp);
    }
  };
  HIPCHK(hipMemsetAsync(d_in, 0, ncell, st));
  for (const vdn_box &gb : la->boxes[s->lev]) {
    Range3 r; for (int d = 0; d < 3; d++) { r.lo[d] = gb.lo[d] - pd.lo[d]; r.hi[d] = gb.hi[d] - pd.lo[d]; }
    hipLaunchKernelGGL(kk_fill_bytes, grid_for(r), dim3(64, 4, 1), 0, st, d_in, n[0], n[1], r);
  }
  sweep(d_tags, d_tmp, buf_wid, 1);
  sweep(d_in, d_tmp, nest, 0);
  // 3. cluster on the lattice of blocks; a block takes part only if it lies in the nesting region as a whole (a tagged cell outside the nesting region
  // cannot tag a block: the block is then not inside as a whole either)
  const size_t nblk = (size_t)G.n[0] * G.n[1] * G.n[2];
  G.t.assign(nblk, 0); G.ok.assign(nblk, 0);
  const int bz = dm == 3 ? blocking : 1;
  {
    DevBytes lat; lat.alloc(2 * nblk);
    unsigned char *d_lat = lat.p;
    Range3 rb; for (int d = 0; d < 3; d++) { rb.lo[d] = 0; rb.hi[d] = G.n[d] - 1; }
    hipLaunchKernelGGL(kk_block_lattice, grid_for(rb), dim3(64, 4, 1), 0, st, (const unsigned char *)d_tags, (const unsigned char *)d_in, d_lat, d_lat + nblk,
                       n[0], n[1], G.n[0], G.n[1], blocking, bz, rb);
    HIPCHK(hipMemcpyAsync(G.t.data(), d_lat, nblk, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(G.ok.data(), d_lat + nblk, nblk, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  }
  { unsigned char *p = tags.p; tags.p = nullptr; HIPCHK(hipFree(p)); }      // (the bitmap goes before the host half, as the other three just did)
  std::vector<IBox> cl;
  IBox whole; for (int d = 0; d < 3; d++) { whole.lo[d] = 0; whole.hi[d] = G.n[d] - 1; }
  cluster(G, whole, min_eff, std::max(1, (min_width + blocking - 1) / blocking), cl);
  // 3b. merge neighbours whose union is again a box (cluster.h)
  merge_boxes(cl);
  // 4. refine (blocks -> cells of this level -> cells of the finer level) and chop to max_grid_size
  std::vector<vdn_box> out;
  for (const IBox &b : cl) {
    int flo[3], fhi[3], cnt[3], len[3];
    for (int d = 0; d < 3; d++) {
      const int bl = d < dm ? blocking : 1, rr = d < dm ? 2 : 1;
      flo[d] = (pd.lo[d] + b.lo[d] * bl) * rr; fhi[d] = (pd.lo[d] + (b.hi[d] + 1) * bl) * rr - 1;
      len[d] = fhi[d] - flo[d] + 1;
      cnt[d] = (len[d] + max_grid_size - 1) / max_grid_size;
    }
    for (int c = 0; c < cnt[2]; c++) for (int bb = 0; bb < cnt[1]; bb++) for (int a = 0; a < cnt[0]; a++) {
      const int q[3] = { a, bb, c };
      vdn_box o;
      for (int d = 0; d < 3; d++) {
        // equal pieces, multiples of the (refined) blocking factor
        const int unit = d < dm ? 2 * blocking : 1, units = len[d] / unit;
        const int u0 = (int)((long)units * q[d] / cnt[d]), u1 = (int)((long)units * (q[d] + 1) / cnt[d]);
        o.lo[d] = flo[d] + u0 * unit; o.hi[d] = flo[d] + u1 * unit - 1;
      }
      out.push_back(o);
    }
  }
  REQUIRE((int)out.size() <= maxboxes, "%s: %d boxes, room for %d", who, (int)out.size(), maxboxes);
  for (size_t i = 0; i < out.size(); i++) boxes_out[i] = out[i];
  *nboxes_out = (int)out.size();
}

// s: the state of ONE level (valid cells of its local boxes).  boxes_out: boxes of the next finer level in ITS index space
extern "C" int vdn_make_new_grids(const vdn_multifab *s, int lev1, int buf_wid, int nest, double min_eff, int min_width, int blocking,
                                  int max_grid_size, int maxboxes, vdn_box *boxes_out, int *nboxes_out, long *ntagged) {
  VDN_TRY
  check_grid_args("vdn_make_new_grids", s, min_width, blocking, max_grid_size, boxes_out, nboxes_out);
  // 1. tags on the device (tag_boxes.f90:142-210: thresholds by level, prob_type)
  DevBytes tags;
  tag_level(s, lev1, tags);
  new_grids_from_tags("vdn_make_new_grids", s, tags, buf_wid, nest, min_eff, min_width, blocking, max_grid_size, maxboxes, boxes_out, nboxes_out, ntagged);
  VDN_CATCH
}
// the same with step 1 by criteria (tag_level_by)
extern "C" int vdn_make_new_grids_by(const vdn_multifab *s, vdn_multifab *u, const double *dx, const vdn_bc_tower *bct, int lev1,
                                     int ncrit, const vdn_tag_criterion *crit,
                                     int buf_wid, int nest, double min_eff, int min_width, int blocking,
                                     int max_grid_size, int maxboxes, vdn_box *boxes_out, int *nboxes_out, long *ntagged) {
  VDN_TRY
  REQUIRE(ctx().inited, "vdn_init has not been called");
  check_grid_args("vdn_make_new_grids_by", s, min_width, blocking, max_grid_size, boxes_out, nboxes_out);
  DevBytes tags;
  tag_level_by("vdn_make_new_grids_by", s, u, dx, bct, lev1, ncrit, crit, tags);
  new_grids_from_tags("vdn_make_new_grids_by", s, tags, buf_wid, nest, min_eff, min_width, blocking, max_grid_size, maxboxes, boxes_out, nboxes_out, ntagged);
  VDN_CATCH
}
