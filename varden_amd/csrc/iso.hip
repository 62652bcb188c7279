// iso.hip -- where a field of a hierarchy takes a value: vdn_isosurface, vdn_isosurface_write (include/varden_amd.h).  The surface q = iso of a cell-centred field over
// the COMPOSITE grid of vdn_diagnostics by marching tetrahedra, its area, its area vector and the volume above it, and the triangles themselves in a fixed order.  No
// reference counterpart; DESIGN.md section 27.  iso_cell.h holds the whole per-cell routine and states every expression.
//
// Launch form.  The slab cut of diag_plan.h: a workgroup of four waves per slab, the thread -> cell map of composite.h.  The slab order (level, global box, k) with the map's
// cell order (i fastest, then j, then k) IS the output order.
//   pass 1 (kk_iso_sums)  per cell the 3 x 3 x 3 neighbourhood (27 loads), the eight node values, the six masks; a thread adds its cells in ascending order, the waves meet
//            through wave_sum / WaveMeet, ONE partial per quantity goes to the slab's slot: the triangle count, the cut cells, the non-finite cells, the cells (integers
//            held in doubles, exact), the area, the area vector, the volume above.  Several ranks: foreign slots are zero and one sum all-reduce fills them.  kk_iso_final
//            adds the slots in slot order (slot_sum), per level and over all.
//   offsets  the host reads the partials with the results and scans the slabs' triangle counts: every slab gets its base, the same on every rank.
//   pass 2 (kk_iso_write) runs only when triangles were asked for and fit.  A workgroup walks its slab in rounds of 256 consecutive cells; a cell's place is the slab's base
//            plus the running count of the rounds before plus an integer wave scan by shuffles plus the counts of the lower waves from LDS (two buffers by the round's parity:
//            one barrier per round).  A cell's count is the byte kk_iso_sums<true> stored for it when triangles were asked for (form 1, what vdn_isosurface runs: only cut
//            cells load their neighbourhood again), or iso_count on nodes formed again (form 0); vdn_isosurface_timed runs either and times the passes (DESIGN section
//            27 has both measured).  A cut cell forms its nodes (iso_cell) and stores its triangles at its place.  No atomic decides a position.  Several ranks: each writes its own
//            slabs into a zero-filled buffer of the global size and one sum all-reduce fills the rest (x + 0 + ... + 0 is x; coordinates are >= +0).
// Memory: descriptors, masks, partials, bases and the triangle buffer live in the arena of the call's ArenaScope.  The call fills no ghost cell and writes none of its inputs.
#include "composite.h"
#include "iso_cell.h"

namespace {
constexpr int IS_THREADS = COMP_THREADS;
// a slab's partial ...
enum { IQ_NTRI = 0, IQ_CUT, IQ_NONFIN, IQ_CELLS, IQ_AREA, IQ_AV, IQ_VOL = IQ_AV + 3, IQ_N };
// ... and what kk_iso_final leaves: the totals, then ntri, cut cells, cells and area level by level
enum { IO_LEV = IQ_N, IO_N = IO_LEV + 4 * VDN_MAXLEV };
static_assert(IO_N <= 64, "one wave per result, few of them");
static_assert(DIAG_SLAB_CELLS * ISO_MAX_TRI < 0x7fffffffl, "a slab's triangle count fits an int");

// what a level's cells share.  fl / fh: the cell index at which a low / high node lies on a domain face with a face value (INT_MIN: none)
struct IsoLev { double dx[3], vtet, iso; int fl[3], fh[3], comp; };

// the nodes of cell (i, j, k), a valid cell of the piece's box, and their positions
DEVI void iso_load(const FV &f, const IsoLev &L, int i, int j, int k, double (&q)[8], double (&xlo)[3], double (&xhi)[3]) {
  const double *__restrict__ p = f.p + fv_idx(f, i, j, k) + f.sc * L.comp;
  const long sy = f.n0, sz = (long)f.n0 * f.n1;
  double a[27];
  #pragma unroll
  for (int kk = 0; kk < 3; kk++) {
    #pragma unroll
    for (int jj = 0; jj < 3; jj++) {
      #pragma unroll
      for (int ii = 0; ii < 3; ii++) a[ii + 3 * jj + 9 * kk] = p[(ii - 1) + sy * (jj - 1) + sz * (kk - 1)];
    }
  }
  const bool flo[3] = { i == L.fl[0], j == L.fl[1], k == L.fl[2] }, fhi[3] = { i == L.fh[0], j == L.fh[1], k == L.fh[2] };
  iso_nodes(a, flo, fhi, q);
  xlo[0] = (double)i * L.dx[0]; xlo[1] = (double)j * L.dx[1]; xlo[2] = (double)k * L.dx[2];
  xhi[0] = (double)(i + 1) * L.dx[0]; xhi[1] = (double)(j + 1) * L.dx[1]; xhi[2] = (double)(k + 1) * L.dx[2];
}

// STORE: the triangle count of every cell of the slab (0 for a covered or non-finite one) also goes to cnt[cell_off[workgroup] + the cell's number in the slab], for the
// form of pass 2 that reads the counts instead of forming them again
template <bool STORE>
__global__ void __launch_bounds__(IS_THREADS) kk_iso_sums(const CompBox *descs, IsoLev L, double *__restrict__ part, const long *__restrict__ cell_off, unsigned char *__restrict__ cnt) {
  const CompBox &D = as_constant(descs + blockIdx.x);
  const int nx = D.hi[0] - D.lo[0] + 1, ny = D.hi[1] - D.lo[1] + 1, nz = D.hi[2] - D.lo[2] + 1;
  const int tot = nx * ny * nz;
  const unsigned char *mask = D.mask;
  const FV f = D.u;
  double a[IQ_N];
  #pragma unroll
  for (int q = 0; q < IQ_N; q++) a[q] = 0.0;
  int ntri = 0, ncut = 0, nbad = 0, ncell = 0;
  CellMap M(nx, ny, (int)threadIdx.x);
  for (int t0 = (int)threadIdx.x; t0 < tot; t0 += IS_THREADS) {
    const int i = D.lo[0] + M.ci, j = D.lo[1] + M.cj, k = D.lo[2] + M.ck;
    M.step();
    if (!cell_open(D, mask, i, j, k)) {
      if constexpr (STORE) cnt[cell_off[blockIdx.x] + t0] = 0;
      continue;
    }
    double q[8], xlo[3], xhi[3];
    iso_load(f, L, i, j, k, q, xlo, xhi);
    IsoSums S;
    const int n = iso_cell(q, xlo, xhi, L.iso, L.vtet, S, [](const double (&)[3], const double (&)[3], const double (&)[3]) {});
    if constexpr (STORE) cnt[cell_off[blockIdx.x] + t0] = (unsigned char)(n < 0 ? 0 : n);
    ncell++;
    if (n == ISO_NONFINITE) { nbad++; continue; }
    ntri += n; ncut += n > 0 ? 1 : 0;
    a[IQ_AREA] = a[IQ_AREA] + S.area;
    #pragma unroll
    for (int d = 0; d < 3; d++) a[IQ_AV + d] = a[IQ_AV + d] + S.av[d];
    a[IQ_VOL] = a[IQ_VOL] + S.vol;
  }
  a[IQ_NTRI] = (double)ntri; a[IQ_CUT] = (double)ncut; a[IQ_NONFIN] = (double)nbad; a[IQ_CELLS] = (double)ncell;
  #pragma unroll
  for (int q = 0; q < IQ_N; q++) a[q] = wave_sum(a[q]);
  __shared__ WaveMeet<IQ_N, 1> sh;
  const u64 none[1] = { 0 };
  if ((threadIdx.x & 63) == 0) sh.put((int)threadIdx.x >> 6, a, none);
  __syncthreads();
  if ((int)threadIdx.x < IQ_N) part[(long)D.slot * IQ_N + threadIdx.x] = sh.sum((int)threadIdx.x);
}

// one wave per result: the totals over every slot in slot order, then ntri, cut cells, cells and area level by level
struct IsoStart { int start[VDN_MAXLEV + 1]; };
__global__ void __launch_bounds__(64) kk_iso_final(const double *__restrict__ part, IsoStart L, int nlev, double *__restrict__ res) {
  const int t = (int)blockIdx.x, lane = (int)threadIdx.x;
  int q = t, s0 = 0, s1 = L.start[nlev];
  if (t >= IO_LEV) {
    const int g = (t - IO_LEV) / VDN_MAXLEV, n = (t - IO_LEV) % VDN_MAXLEV;
    q = g == 0 ? IQ_NTRI : g == 1 ? IQ_CUT : g == 2 ? IQ_CELLS : IQ_AREA;
    if (n < nlev) { s0 = L.start[n]; s1 = L.start[n + 1]; } else s1 = 0;
  }
  const double v = slot_sum(0.0, part, IQ_N, q, nullptr, s0, s1, lane);
  if (lane == 0) res[t] = v;
}

// STORED: a cell's count is read from cnt (what kk_iso_sums<true> left) and only a cell with triangles loads its neighbourhood; otherwise every cell forms its nodes
// and counts again (iso_count)
template <bool STORED>
__global__ void __launch_bounds__(IS_THREADS) kk_iso_write(const CompBox *descs, IsoLev L, const long long *__restrict__ base, double *__restrict__ tri, long long ntri_all,
                                                           const long *__restrict__ cell_off, const unsigned char *__restrict__ cnt) {
  static_assert(COMP_WAVES == 4, "the carry below names the four waves");
  __shared__ int wsum[2][COMP_WAVES];
  const CompBox &D = as_constant(descs + blockIdx.x);
  const int nx = D.hi[0] - D.lo[0] + 1, ny = D.hi[1] - D.lo[1] + 1, nz = D.hi[2] - D.lo[2] + 1;
  const int tot = nx * ny * nz;
  const unsigned char *mask = D.mask;
  const FV f = D.u;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  long long run = base[D.slot];                        // the place of the round's first triangle
  CellMap M(nx, ny, t);
  // the round loop is uniform over the workgroup: every thread takes part in every shuffle and barrier; a thread past the slab's end has no cell
  for (int t0 = 0, r = 0; t0 < tot; t0 += IS_THREADS, r ^= 1) {
    bool live = t0 + t < tot;
    const int i = D.lo[0] + (live ? M.ci : 0), j = D.lo[1] + (live ? M.cj : 0), k = D.lo[2] + (live ? M.ck : 0);
    M.step();
    double q[8], xlo[3], xhi[3];
    int n = 0;
    if constexpr (STORED) {
      if (live) n = cnt[cell_off[blockIdx.x] + t0 + t];
    } else {
      live = live && cell_open(D, mask, i, j, k);
      if (live) {
        iso_load(f, L, i, j, k, q, xlo, xhi);
        n = iso_count(q, L.iso);
        if (n < 0) n = 0;
      }
    }
    int x = n;                                         // the inclusive scan of the wave
    #pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(x, o, 64); x += lane >= o ? y : 0; }
    if (lane == 63) wsum[r][wave] = x;
    __syncthreads();
    const int w0 = wsum[r][0], w1 = wsum[r][1], w2 = wsum[r][2], w3 = wsum[r][3];
    const int below = wave == 0 ? 0 : wave == 1 ? w0 : wave == 2 ? w0 + w1 : w0 + w1 + w2;
    long long at = run + below + (x - n);
    run += (w0 + w1) + (w2 + w3);
    if (n > 0 && at >= 0 && at + n <= ntri_all) {
      if constexpr (STORED) iso_load(f, L, i, j, k, q, xlo, xhi);
      double *dst = tri + 9 * at;
      IsoSums S;
      iso_cell(q, xlo, xhi, L.iso, L.vtet, S, [&](const double (&p0)[3], const double (&p1)[3], const double (&p2)[3]) {
        #pragma unroll
        for (int d = 0; d < 3; d++) { dst[d] = p0[d]; dst[3 + d] = p1[d]; dst[6 + d] = p2[d]; }
        dst += 9;
      });
    }
  }
}

constexpr int NO_FACE = -2147483647 - 1;

void iso_check(const char *who, int nlev, const vdn_layout *mla, vdn_multifab *const *mf, int comp, int bccomp, const double *dx, const vdn_bc_tower *bct, double iso,
               long long max_tri, const double *tri_host, const vdn_iso *out) {
  REQUIRE(ctx().inited, "%s: vdn_init has not been called", who);
  REQUIRE(mla && mf && out, "%s: null argument (mla, mf, out)", who);
  REQUIRE(nlev >= 1 && nlev <= VDN_MAXLEV, "%s: nlev = %d is outside 1 .. %d", who, nlev, VDN_MAXLEV);
  REQUIRE(nlev == mla->nlev, "%s: nlev = %d does not match the layout's %d levels", who, nlev, mla->nlev);
  REQUIRE(dx, "%s: dx is NULL (positions are physical)", who);
  REQUIRE(bct, "%s: bct is NULL (the boundary types decide where a ghost cell holds a face value)", who);
  REQUIRE(bct->la == mla, "%s: the bc tower belongs to another layout", who);
  REQUIRE(ctx().prm.dm == 3, "%s: dm = %d: surfaces are extracted from 3-D fields only", who, ctx().prm.dm);
  REQUIRE(iso_finite(iso), "%s: iso = %g is not finite", who, iso);
  REQUIRE(max_tri >= 0, "%s: max_tri = %lld is negative", who, max_tri);
  REQUIRE(max_tri == 0 || tri_host, "%s: max_tri = %lld with a NULL tri_host", who, max_tri);
  REQUIRE(comp >= 0, "%s: comp = %d is negative", who, comp);
  REQUIRE(bccomp >= 0 && bccomp < bct->ncomp_adv, "%s: boundary component %d, the tower holds %d", who, bccomp, bct->ncomp_adv);
  for (int n = 0; n < nlev; n++) {
    for (int d = 0; d < 3; d++) REQUIRE(dx[3 * n + d] > 0.0 && dx[3 * n + d] < __builtin_huge_val(), "%s: level %d: dx[%d] = %g", who, n, d, dx[3 * n + d]);
    REQUIRE(mf[n], "%s: level %d: null multifab", who, n);
    REQUIRE(mf[n]->la == mla && mf[n]->lev == n, "%s: level %d: mf is not a multifab of level %d of mla", who, n, n);
    for (int d = 0; d < 3; d++) REQUIRE(!mf[n]->nodal[d], "%s: level %d: mf is nodal; cell-centred multifabs expected", who, n);
    REQUIRE(mf[n]->nc > comp, "%s: level %d: mf carries %d components, component %d asked for", who, n, mf[n]->nc, comp);
    REQUIRE(mf[n]->ng >= 1, "%s: level %d: mf has no ghost layer (the node values read one)", who, n);
    REQUIRE(mla->pd[n].lo[0] == 0 && mla->pd[n].lo[1] == 0 && mla->pd[n].lo[2] == 0, "%s: the domain's low corner must be cell 0 (prob_lo = 0)", who);
    if (n < nlev - 1) for (int d = 0; d < 3; d++) REQUIRE(mla->rr[3 * n + d] == 2, "%s: level %d: a refinement ratio of 2 is expected (it is %d along %d)", who, n, mla->rr[3 * n + d], d);
  }
}
}   // namespace

extern "C" size_t vdn_iso_sizeof(void) { return sizeof(vdn_iso); }

namespace {
// what pass 2 does when the library chooses: ISO_RECOMPUTE or ISO_STORED (DESIGN section 27 has both measured)
constexpr int ISO_RECOMPUTE = 0, ISO_STORED = 1, ISO_DEFAULT_FORM = ISO_STORED;
struct IsoTimer {       // device time of a run of launches, for vdn_isosurface_timed alone
  hipEvent_t a = nullptr, b = nullptr; bool on;
  explicit IsoTimer(bool on_) : on(on_) { if (on) { HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b)); } }
  ~IsoTimer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  void start(hipStream_t st) { if (on) HIPCHK(hipEventRecord(a, st)); }
  void stop(hipStream_t st) { if (on) HIPCHK(hipEventRecord(b, st)); }
  double ms() { float t = 0.0f; if (on) { HIPCHK(hipEventSynchronize(b)); HIPCHK(hipEventElapsedTime(&t, a, b)); } return (double)t; }
};

void iso_run(const char *who, int nlev, vdn_layout *mla, vdn_multifab *const *mf, int comp, int bccomp, const double *dx, const vdn_bc_tower *bct, double iso,
             long long max_tri, double *tri_host, unsigned char *lev_host, vdn_iso *out, int form, double *ms) {
  iso_check(who, nlev, mla, mf, comp, bccomp, dx, bct, iso, max_tri, tri_host, out);
  REQUIRE(form == ISO_RECOMPUTE || form == ISO_STORED, "%s: form = %d (0: pass 2 recomputes, 1: pass 2 reads stored counts)", who, form);
  const bool stored = form == ISO_STORED && tri_host && max_tri > 0;
  IsoTimer t1(ms != nullptr), t2(ms != nullptr);
  if (ms) ms[0] = ms[1] = 0.0;
  hipStream_t st = ctx().stream;
  ArenaScope arena;
  IsoStart LS;
  const std::vector<DiagSlab> slabs = diag_plan(nlev, mla->boxes.data(), LS.start);
  const int nslab = LS.start[nlev];
  REQUIRE(nslab > 0, "%s: the hierarchy holds no cell", who);
  // one array of doubles: the partials [nslab][IQ_N], then the results
  const size_t npart = (size_t)nslab * IQ_N;
  double *d_part = (double *)arena_alloc(sizeof(double) * (npart + IO_N));
  double *d_res = d_part + npart;
  const bool ranks = comm_active();
  if (ranks) HIPCHK(hipMemsetAsync(d_part, 0, sizeof(double) * npart, st));
  IsoLev L[VDN_MAXLEV]; const CompBox *d_desc[VDN_MAXLEV]; int nd[VDN_MAXLEV]; double vol[VDN_MAXLEV];
  std::vector<long> off[VDN_MAXLEV]; long *d_off[VDN_MAXLEV]; long ncnt = 0;
  for (int n = 0; n < nlev; n++) {
    for (int d = 0; d < 3; d++) {
      L[n].dx[d] = dx[3 * n + d];
      L[n].fl[d] = bct->adv_bc(n, 0, d, 0, bccomp) == VDN_EXT_DIR ? mla->pd[n].lo[d] : NO_FACE;
      L[n].fh[d] = bct->adv_bc(n, 0, d, 1, bccomp) == VDN_EXT_DIR ? mla->pd[n].hi[d] : NO_FACE;
    }
    vol[n] = cell_volume(dx, n, 3);
    L[n].vtet = vol[n] / 6.0; L[n].iso = iso; L[n].comp = comp;
    d_desc[n] = nullptr; nd[n] = 0; d_off[n] = nullptr;
    const std::vector<CompPiece> mine = slab_pieces(slabs, n, mla);
    if (mine.empty()) continue;
    d_desc[n] = composite_level(who, n, nlev, mla, mf, mf, mine);
    nd[n] = (int)mine.size();
    for (const CompPiece &P : mine) { off[n].push_back(ncnt); ncnt += (long)(P.hi[0] - P.lo[0] + 1) * (P.hi[1] - P.lo[1] + 1) * (P.hi[2] - P.lo[2] + 1); }
  }
  unsigned char *d_cnt = nullptr;
  if (stored) {
    d_cnt = (unsigned char *)arena_alloc((size_t)ncnt);
    for (int n = 0; n < nlev; n++) if (nd[n] > 0) { d_off[n] = (long *)arena_alloc(sizeof(long) * off[n].size()); upload_staged(d_off[n], off[n].data(), sizeof(long) * off[n].size()); }
  }
  t1.start(st);
  for (int n = 0; n < nlev; n++) {
    if (nd[n] == 0) continue;
    if (stored) hipLaunchKernelGGL(kk_iso_sums<true>, dim3(nd[n]), dim3(IS_THREADS), 0, st, d_desc[n], L[n], d_part, (const long *)d_off[n], d_cnt);
    else        hipLaunchKernelGGL(kk_iso_sums<false>, dim3(nd[n]), dim3(IS_THREADS), 0, st, d_desc[n], L[n], d_part, (const long *)nullptr, (unsigned char *)nullptr);
  }
  t1.stop(st);
  if (ranks) comm_allreduce_sum_dev(d_part, npart);
  hipLaunchKernelGGL(kk_iso_final, dim3(IO_N), dim3(64), 0, st, (const double *)d_part, LS, nlev, d_res);
  std::vector<double> h(npart + IO_N);
  HIPCHK(hipMemcpyAsync(h.data(), d_part, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  const double *r = h.data() + npart;
  vdn_iso R; memset(&R, 0, sizeof R);
  R.ntri = (long long)r[IQ_NTRI]; R.cut_cells = (long long)r[IQ_CUT]; R.nonfinite_cells = (long long)r[IQ_NONFIN];
  R.area = r[IQ_AREA]; R.volume_above = r[IQ_VOL];
  for (int d = 0; d < 3; d++) R.area_vec[d] = r[IQ_AV + d];
  for (int n = 0; n < nlev; n++) {
    R.ntri_lev[n] = (long long)r[IO_LEV + n]; R.cut_cells_lev[n] = (long long)r[IO_LEV + VDN_MAXLEV + n]; R.area_lev[n] = r[IO_LEV + 3 * VDN_MAXLEV + n];
    // the cells that were cut up: all but the non-finite ones, level by level, each with its level's volume
    long long bad = 0;
    for (int s = LS.start[n]; s < LS.start[n + 1]; s++) bad += (long long)h[(size_t)s * IQ_N + IQ_NONFIN];
    R.volume = R.volume + (double)((long long)r[IO_LEV + 2 * VDN_MAXLEV + n] - bad) * vol[n];
  }
  if (tri_host && R.ntri > 0 && R.ntri <= max_tri) {
    std::vector<long long> base((size_t)nslab);
    long long at = 0;
    for (int s = 0; s < nslab; s++) { base[s] = at; at += (long long)h[(size_t)s * IQ_N + IQ_NTRI]; }
    REQUIRE(at == R.ntri, "%s: the slabs hold %lld triangles, the sum says %lld", who, at, R.ntri);
    const size_t nval = 9 * (size_t)R.ntri;
    long long *d_base = (long long *)arena_alloc(sizeof(long long) * (size_t)nslab);
    double *d_tri = (double *)arena_alloc(sizeof(double) * nval);
    upload_staged(d_base, base.data(), sizeof(long long) * (size_t)nslab);
    if (ranks) HIPCHK(hipMemsetAsync(d_tri, 0, sizeof(double) * nval, st));
    t2.start(st);
    for (int n = 0; n < nlev; n++) {
      if (nd[n] == 0) continue;
      if (stored) hipLaunchKernelGGL(kk_iso_write<true>, dim3(nd[n]), dim3(IS_THREADS), 0, st, d_desc[n], L[n], (const long long *)d_base, d_tri, R.ntri, (const long *)d_off[n], (const unsigned char *)d_cnt);
      else        hipLaunchKernelGGL(kk_iso_write<false>, dim3(nd[n]), dim3(IS_THREADS), 0, st, d_desc[n], L[n], (const long long *)d_base, d_tri, R.ntri, (const long *)nullptr, (const unsigned char *)nullptr);
    }
    t2.stop(st);
    if (ranks) comm_allreduce_sum_dev(d_tri, nval);
    HIPCHK(hipMemcpyAsync(tri_host, d_tri, sizeof(double) * nval, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (lev_host) {
      size_t t = 0;
      for (int n = 0; n < nlev; n++) for (long long e = 0; e < R.ntri_lev[n]; e++) lev_host[t++] = (unsigned char)n;
    }
    R.written = R.ntri;
    if (ms) ms[1] = t2.ms();
  }
  if (ms) ms[0] = t1.ms();
  arena.release();
  *out = R;
}
}   // namespace

extern "C" int vdn_isosurface(int nlev, vdn_layout *mla, vdn_multifab *const *mf, int comp, int bccomp, const double *dx, const vdn_bc_tower *bct, double iso,
                              long long max_tri, double *tri_host, unsigned char *lev_host, vdn_iso *out) {
  VDN_TRY
  iso_run("vdn_isosurface", nlev, mla, mf, comp, bccomp, dx, bct, iso, max_tri, tri_host, lev_host, out, ISO_DEFAULT_FORM, nullptr);
  VDN_CATCH
}

// the same call with the form of pass 2 chosen by the caller and the device time of the two passes' launches (hipEvents around them, no read-back inside): the
// measurement behind the choice of ISO_DEFAULT_FORM.  Both forms give the same bits
extern "C" int vdn_isosurface_timed(int nlev, vdn_layout *mla, vdn_multifab *const *mf, int comp, int bccomp, const double *dx, const vdn_bc_tower *bct, double iso,
                                    long long max_tri, double *tri_host, unsigned char *lev_host, vdn_iso *out, int form, double *ms) {
  VDN_TRY
  REQUIRE(ms, "vdn_isosurface_timed: null argument (ms)");
  iso_run("vdn_isosurface_timed", nlev, mla, mf, comp, bccomp, dx, bct, iso, max_tri, tri_host, lev_host, out, form, ms);
  VDN_CATCH
}

// binary PLY, little endian: a triangle soup, three vertices per face, no vertex merged; rank 0 writes.  A host function: it touches no device and runs before vdn_init
// too (the rank is then 0)
extern "C" int vdn_isosurface_write(const char *path, long long ntri, const double *tri_host, const unsigned char *lev_host, double iso, double time) {
  try {
  REQUIRE(path, "vdn_isosurface_write: null argument (path)");
  REQUIRE(ntri >= 0 && 3 * ntri <= 0x7fffffffll, "vdn_isosurface_write: ntri = %lld (0 .. %lld: a face indexes its vertices with 32-bit integers)", ntri, 0x7fffffffll / 3);
  REQUIRE(ntri == 0 || (tri_host && lev_host), "vdn_isosurface_write: %lld triangles need tri_host and lev_host", ntri);
  if (ctx().rank != 0) return 0;
  FILE *f = fopen(path, "wb");
  REQUIRE(f, "vdn_isosurface_write: cannot open %s", path);
  fprintf(f, "ply\nformat binary_little_endian 1.0\ncomment VDN_ISO 1 iso %.17g time %.17g\nelement vertex %lld\nproperty double x\nproperty double y\nproperty double z\n"
             "element face %lld\nproperty list uchar int vertex_indices\nproperty uchar level\nend_header\n", iso, time, 3 * ntri, ntri);
  bool ok = ntri == 0 || fwrite(tri_host, sizeof(double), 9 * (size_t)ntri, f) == 9 * (size_t)ntri;
  std::vector<unsigned char> faces(14 * (size_t)ntri);
  for (long long t = 0; t < ntri; t++) {
    unsigned char *p = faces.data() + 14 * (size_t)t;
    p[0] = 3;
    for (int v = 0; v < 3; v++) { const int idx = (int)(3 * t + v); memcpy(p + 1 + 4 * v, &idx, 4); }
    p[13] = lev_host[t];
  }
  ok = ok && (ntri == 0 || fwrite(faces.data(), 1, faces.size(), f) == faces.size());
  ok = (fclose(f) == 0) && ok;
  REQUIRE(ok, "vdn_isosurface_write: writing %s failed", path);
  } catch (const std::exception &e) { vdn_set_error("%s", e.what()); return 1; }
  return 0;
}
