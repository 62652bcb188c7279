// profiles.hip -- plane-averaged profiles of a hierarchy on the device: vdn_profiles, vdn_profiles_layout, vdn_profiles_nbins (include/varden_amd.h).  No reference
// counterpart.  DESIGN.md section 22 defines every row.
//
// Definition.  nlev levels, axis a, L = nlev - 1 the finest level OF THE HIERARCHY.  Bins are the planes of level L's index space along a: nbins = ncells_a(level 0)
// << L, bin m is m h <= x_a < (m + 1) h with h = dx[L][a].  The sums run over the composite grid of vdn_diagnostics: the valid cells of level l that no box of level
// l + 1 covers.  Such a cell with index i_a lies in the r = 1 << (L - l) bins i_a r .. i_a r + r - 1 and contributes to EACH with the weight w_l = (dx dy dz of level
// l) / r (dm = 2: dx dy / r), formed once per level on the host.  Per bin and row the term named in varden_amd.h is summed: products associated left to right, then
// multiplied by w_l; `volume` is (the bin's composite cells of level l) * w_l, added over the levels; extrema are exact, through the order-preserving key of vdn_dev.h.
//
// Launch form.  profile_plan.h cuts every box into pieces and gives every piece one SLOT of partials per cell index along a, numbered in (level, global box, piece)
// order.  One launch per level, kk_profile<NS, AXIS>:
//   AXIS = 0      a workgroup takes a piece (<= 64 cells along x, a run of k-planes); lane i of every wave owns the index lo + i and walks the piece's (j, k) rows
//                 wave, wave + 4, ... in ascending order -- no cross-lane step; the four waves of a lane meet as (w0 + w1) + (w2 + w3) through LDS
//   AXIS = 1, 2   a workgroup takes one cross-section of a piece (one index along a): per-thread accumulation in the thread -> cell map, the shuffle tree and
//                 the (w0 + w1) + (w2 + w3) LDS step of composite.h
// and stores ONE partial per column into the slot.  Sums are doubles, an extremum travels as its 64-bit key cut into two halves that a double holds exactly (a minimum
// as the complement, so that an empty slot is 0), the cell count as a double.  Several ranks: the slots of foreign boxes are zero and ONE sum all-reduce of the slot
// array fills them.  kk_profile_final then gives a wave to every (bin, row): starting from +0 it adds, level by level, the slots the level's table names for the index
// m >> (L - l), in table order (slot_sum); key rows take the maximum (slot_max).  No floating-point atomic anywhere: the bits of a result depend on the box lists
// alone -- not on the number of ranks, not on the call; composite.h states what that rests on.
// Memory: descriptors, tables, partials, the covered-cell masks and the result live in the arena of the call's ArenaScope; one copy brings rows and counts home.  The call writes none of its inputs and reads no ghost cell.
#include "composite.h"
#include "profile_plan.h"

namespace {
constexpr int PF_THREADS = COMP_THREADS, PF_MAXS = 11, PF_MAXROW = 80;
static_assert(PROF_MAXLEV == VDN_MAXLEV && PROF_XW == 64, "profile_plan.h and the kernels");

// the columns of a slot's partial in an instantiation that carries NS scalars and three velocity components (unused ones stay 0); ruu: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2)
template <int NS> struct PT {
  enum { VOL = 0, S = 1, SS = S + NS, U = SS + NS, RU = U + 3, RUU = RU + 3, SUA = RUU + 6, NSUM = SUA + NS - 1,
         K_SMIN = 0, K_SMAX = NS, K_UMIN = 2 * NS, K_UMAX = 2 * NS + 3, NKEY = 2 * NS + 6,
         KEYS = NSUM, CELLS = NSUM + 2 * NKEY, PQ = CELLS + 1, NQ = NSUM + NKEY };
  static_assert(NSUM <= 64 && NKEY <= 64, "one thread per column in the last step of a workgroup");
};
constexpr int ruu_col(int d, int e) { return d * 3 - d * (d - 1) / 2 + (e - d); }

template <int NS, int AXIS> struct Acc {
  double a[PT<NS>::NSUM]; u64 kx[PT<NS>::NKEY]; int ncell;
  DEVI void zero() {
    #pragma unroll
    for (int q = 0; q < PT<NS>::NSUM; q++) a[q] = 0.0;
    #pragma unroll
    for (int q = 0; q < PT<NS>::NKEY; q++) kx[q] = 0;
    ncell = 0;
  }
  // one composite cell: every term is (product, left to right) * w
  DEVI void add(const double (&u)[3], const double (&s)[NS], int nscal, int dm, double w) {
    typedef PT<NS> T;
    ncell++;
    #pragma unroll
    for (int c = 0; c < NS; c++) if (c < nscal) {
      a[T::S + c] = a[T::S + c] + s[c] * w;
      a[T::SS + c] = a[T::SS + c] + (s[c] * s[c]) * w;
      if (c >= 1) a[T::SUA + (c >= 1 ? c - 1 : 0)] = a[T::SUA + (c >= 1 ? c - 1 : 0)] + (s[c] * u[AXIS]) * w;
      const u64 key = key_of(s[c]);
      kx[T::K_SMIN + c] = key_max(kx[T::K_SMIN + c], ~key); kx[T::K_SMAX + c] = key_max(kx[T::K_SMAX + c], key);
    }
    #pragma unroll
    for (int d = 0; d < 3; d++) if (d < dm) {
      a[T::U + d] = a[T::U + d] + u[d] * w;
      const double ru = s[0] * u[d];
      a[T::RU + d] = a[T::RU + d] + ru * w;
      #pragma unroll
      for (int e = d; e < 3; e++) if (e < dm) a[T::RUU + ruu_col(d, e)] = a[T::RUU + ruu_col(d, e)] + (ru * u[e]) * w;
      const u64 key = key_of(u[d]);
      kx[T::K_UMIN + d] = key_max(kx[T::K_UMIN + d], ~key); kx[T::K_UMAX + d] = key_max(kx[T::K_UMAX + d], key);
    }
  }
};

// NS: the scalars the instantiation can carry (nscal <= NS; the loops over them are unrolled so that every accumulator is a register).
// AXIS = 0: one workgroup per piece (start unused); AXIS = 1, 2: one per (piece, index along the axis), start[p]: the first workgroup of piece p
template <int NS, int AXIS>
__global__ void __launch_bounds__(PF_THREADS) kk_profile(const CompBox *descs, const int *start, int npiece, double *__restrict__ part, int nscal, int dm, double w) {
  typedef PT<NS> T;
  constexpr int UNR = NS <= 4 ? 4 : 2;                   // cells per thread and trip whose loads are all issued before the first is used
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  Acc<NS, AXIS> A; A.zero();
  if constexpr (AXIS == 0) {
    const CompBox &D = as_constant(descs + blockIdx.x);
    const unsigned char *mask = D.mask;
    const FV fu = D.u, fs = D.s;
    const bool ilive = D.lo[0] + lane <= D.hi[0];
    const int i = ilive ? D.lo[0] + lane : D.lo[0];
    const int ny = D.hi[1] - D.lo[1] + 1, nz = D.hi[2] - D.lo[2] + 1, rows = ny * nz;
    RowMap M(ny, wave, COMP_WAVES);                       // row r of the piece is (r % ny, r / ny); a wave's rows are 4 apart
    for (int r0 = wave; r0 < rows; r0 += 4 * UNR) {
      double uv[UNR][3], sv[UNR][NS]; bool live[UNR];
      #pragma unroll
      for (int e = 0; e < UNR; e++) {
        const bool rl = r0 + 4 * e < rows;
        const int j = D.lo[1] + (rl ? M.ci : 0), k = D.lo[2] + (rl ? M.cr : 0);
        M.step();
        live[e] = load_cell<NS>(D, fu, fs, mask, i, j, k, rl && ilive, nscal, dm, uv[e], sv[e]);
      }
      #pragma unroll
      for (int e = 0; e < UNR; e++) if (live[e]) A.add(uv[e], sv[e], nscal, dm, w);
    }
    A.a[T::VOL] = (double)A.ncell;
    // the four waves of every lane: (w0 + w1) + (w2 + w3) through LDS, CH columns at a time; then a thread per (lane's slot, column)
    constexpr int CH = 8;
    __shared__ double sh[CH][PF_THREADS / 64][64];
    #pragma unroll
    for (int qb = 0; qb < T::NQ; qb += CH) {
      #pragma unroll
      for (int qq = 0; qq < CH; qq++) {
        const int q = qb + qq;
        if (q < T::NSUM) sh[qq][wave][lane] = A.a[q < T::NSUM ? q : 0];
        else if (q < T::NQ) sh[qq][wave][lane] = __longlong_as_double((long long)A.kx[q >= T::NSUM && q < T::NQ ? q - T::NSUM : 0]);
      }
      __syncthreads();
      for (int o = t; o < CH * 64; o += PF_THREADS) {
        const int li = o / CH, qq = o % CH, q = qb + qq;
        if (q >= T::NQ || D.lo[0] + li > D.hi[0]) continue;
        double *out = part + (long)(D.slot + li) * T::PQ;
        if (q < T::NSUM) {
          const double v = sum4(sh[qq][0][li], sh[qq][1][li], sh[qq][2][li], sh[qq][3][li]);
          if (q == T::VOL) { out[T::CELLS] = v; out[T::VOL] = v * w; } else out[q] = v;
        } else {
          key_split(max4((u64)__double_as_longlong(sh[qq][0][li]), (u64)__double_as_longlong(sh[qq][1][li]), (u64)__double_as_longlong(sh[qq][2][li]),
                         (u64)__double_as_longlong(sh[qq][3][li])), out + T::KEYS + 2 * (q - T::NSUM));
        }
      }
      __syncthreads();
    }
  } else {
    constexpr int C = AXIS == 2 ? 1 : 2;                  // the direction the cross-section extends along besides x
    int p = 0;
    { int hi = npiece - 1; const int bid = (int)blockIdx.x;
      while (p < hi) { const int mid = (p + hi + 1) >> 1; if (as_constant(start + mid) <= bid) p = mid; else hi = mid - 1; } }
    const CompBox &D = as_constant(descs + p);
    const int off = (int)blockIdx.x - as_constant(start + p), ia = D.lo[AXIS] + off;
    const unsigned char *mask = D.mask;
    const FV fu = D.u, fs = D.s;
    const int nx = D.hi[0] - D.lo[0] + 1, nr = D.hi[C] - D.lo[C] + 1, tot = nx * nr;
    RowMap M(nx, t);                                      // the cell of index e is (e % nx, e / nx) from the cross-section's corner
    for (int t0 = t; t0 < tot; t0 += UNR * PF_THREADS) {
      double uv[UNR][3], sv[UNR][NS]; bool live[UNR];
      #pragma unroll
      for (int e = 0; e < UNR; e++) {
        const bool cl = t0 + e * PF_THREADS < tot;
        const int i = D.lo[0] + (cl ? M.ci : 0), r = D.lo[C] + (cl ? M.cr : 0);
        M.step();
        const int j = AXIS == 1 ? ia : r, k = AXIS == 1 ? r : ia;
        live[e] = load_cell<NS>(D, fu, fs, mask, i, j, k, cl, nscal, dm, uv[e], sv[e]);
      }
      #pragma unroll
      for (int e = 0; e < UNR; e++) if (live[e]) A.add(uv[e], sv[e], nscal, dm, w);
    }
    A.a[T::VOL] = (double)A.ncell;
    // the wave, then the four waves through LDS, one thread per column
    #pragma unroll
    for (int q = 0; q < T::NSUM; q++) A.a[q] = wave_sum(A.a[q]);
    #pragma unroll
    for (int q = 0; q < T::NKEY; q++) A.kx[q] = wave_max(A.kx[q]);
    __shared__ WaveMeet<T::NSUM, T::NKEY> sh;
    if (lane == 0) sh.put(wave, A.a, A.kx);
    __syncthreads();
    double *out = part + (long)(D.slot + off) * T::PQ;
    if (t < T::NSUM) {
      const double v = sh.sum(t);
      if (t == T::VOL) { out[T::CELLS] = v; out[T::VOL] = v * w; } else out[t] = v;
    } else if (t >= 64 && t < 64 + T::NKEY) key_split(sh.max(t - 64), out + T::KEYS + 2 * (t - 64));
  }
}

// per level the CSR table of profile_plan.h on the device; per output row (and, last, the cell count) the column of the partial and what to do with it
struct ProfTab { const int *ptr[VDN_MAXLEV], *idx[VDN_MAXLEV]; int nlev; };
enum { PK_SUM = 0, PK_MIN = 1, PK_MAX = 2, PK_CELLS = 3 };
struct ProfRows { short col[PF_MAXROW]; unsigned char kind[PF_MAXROW]; };

// a wave per (bin, row): wave g takes bin g / nq, row g % nq (row nq - 1: the cell count)
__global__ void __launch_bounds__(PF_THREADS) kk_profile_final(const double *__restrict__ part, int pq, ProfTab T, ProfRows R, int nq, long nbins,
                                                               double *__restrict__ out, long long *__restrict__ cells) {
  const long g = (long)blockIdx.x * (PF_THREADS / 64) + ((int)threadIdx.x >> 6);
  const int lane = (int)threadIdx.x & 63;
  if (g >= nbins * nq) return;
  const long m = g / nq;
  const int r = (int)(g - m * nq), col = R.col[r], kind = R.kind[r], L = T.nlev - 1;
  if (kind == PK_SUM || kind == PK_CELLS) {
    double v = 0.0;
    for (int l = 0; l <= L; l++) {
      const long ci = m >> (L - l);
      v = slot_sum(v, part, pq, col, T.idx[l], T.ptr[l][ci], T.ptr[l][ci + 1], lane);
    }
    if (lane == 0) { if (kind == PK_CELLS) cells[m] = (long long)v; else out[(long)r * nbins + m] = v; }
  } else {
    u64 key = 0;
    for (int l = 0; l <= L; l++) {
      const long ci = m >> (L - l);
      key = slot_max(key, part, pq, col, T.idx[l], T.ptr[l][ci], T.ptr[l][ci + 1], lane);
    }
    key = wave_max(key);
    if (lane == 0) out[(long)r * nbins + m] = extremum_value(key, kind == PK_MIN);
  }
}

template <int NS> void launch_profile(int axis, int nblock, const CompBox *d, const int *start, int npiece, double *part, int nscal, int dm, double w) {
  hipStream_t st = ctx().stream;
  if (axis == 0)      hipLaunchKernelGGL((kk_profile<NS, 0>), dim3(nblock), dim3(PF_THREADS), 0, st, d, start, npiece, part, nscal, dm, w);
  else if (axis == 1) hipLaunchKernelGGL((kk_profile<NS, 1>), dim3(nblock), dim3(PF_THREADS), 0, st, d, start, npiece, part, nscal, dm, w);
  else                hipLaunchKernelGGL((kk_profile<NS, 2>), dim3(nblock), dim3(PF_THREADS), 0, st, d, start, npiece, part, nscal, dm, w);
}

// the columns of the partial behind every output row of vdn_profile_layout's order, then the cell count
template <int NS> int profile_rows(int dm, int nscal, ProfRows &R) {
  typedef PT<NS> T;
  int n = 0;
  auto put = [&](int col, int kind) { R.col[n] = (short)col; R.kind[n] = (unsigned char)kind; n++; };
  put(T::VOL, PK_SUM);
  for (int c = 0; c < nscal; c++) put(T::S + c, PK_SUM);
  for (int c = 0; c < nscal; c++) put(T::SS + c, PK_SUM);
  for (int d = 0; d < dm; d++) put(T::U + d, PK_SUM);
  for (int d = 0; d < dm; d++) put(T::RU + d, PK_SUM);
  for (int d = 0; d < dm; d++) for (int e = d; e < dm; e++) put(T::RUU + ruu_col(d, e), PK_SUM);
  for (int c = 1; c < nscal; c++) put(T::SUA + c - 1, PK_SUM);
  for (int c = 0; c < nscal; c++) put(T::KEYS + 2 * (T::K_SMIN + c), PK_MIN);
  for (int c = 0; c < nscal; c++) put(T::KEYS + 2 * (T::K_SMAX + c), PK_MAX);
  for (int d = 0; d < dm; d++) put(T::KEYS + 2 * (T::K_UMIN + d), PK_MIN);
  for (int d = 0; d < dm; d++) put(T::KEYS + 2 * (T::K_UMAX + d), PK_MAX);
  put(T::CELLS, PK_CELLS);
  return n;
}

bool layout_of(int dm, int nscal, vdn_profile_layout *lay) {
  if (!lay || (dm != 2 && dm != 3) || nscal < 1 || nscal > PF_MAXS) return false;
  lay->volume = 0; lay->s = 1; lay->ss = lay->s + nscal; lay->u = lay->ss + nscal; lay->ru = lay->u + dm; lay->ruu = lay->ru + dm;
  lay->sua = lay->ruu + dm * (dm + 1) / 2; lay->s_min = lay->sua + nscal - 1; lay->s_max = lay->s_min + nscal; lay->u_min = lay->s_max + nscal;
  lay->u_max = lay->u_min + dm; lay->nrow = lay->u_max + dm;
  return true;
}
}   // namespace

extern "C" size_t vdn_profile_layout_sizeof(void) { return sizeof(vdn_profile_layout); }

extern "C" int vdn_profiles_layout(int dm, int nscal, vdn_profile_layout *lay) {
  if (layout_of(dm, nscal, lay)) return 0;
  vdn_set_error("vdn_profiles_layout: dm = %d (2 or 3), nscal = %d (1 .. %d), lay %s", dm, nscal, PF_MAXS, lay ? "given" : "NULL");
  return 1;
}

extern "C" long vdn_profiles_nbins(int nlev, vdn_layout *mla, int axis) {
  const char *why = nullptr;
  if (!mla) why = "mla is NULL";
  else if (nlev < 1 || nlev > VDN_MAXLEV || nlev != mla->nlev) why = "nlev is outside 1 .. 4 or not the layout's";
  else if (axis < 0 || axis > 2 || (ctx().inited && axis >= ctx().prm.dm)) why = "axis is outside 0 .. dm-1";
  if (why) { vdn_set_error("vdn_profiles_nbins: %s (nlev = %d, axis = %d)", why, nlev, axis); return -1; }
  return (long)(mla->pd[0].hi[axis] - mla->pd[0].lo[axis] + 1) << (nlev - 1);
}

extern "C" int vdn_profiles(int nlev, vdn_layout *mla, vdn_multifab *const *u, vdn_multifab *const *s, const double *dx, int axis, long nbins,
                            double *out_host, long long *cells_host) {
  VDN_TRY
  composite_check("vdn_profiles", nlev, mla, u, s, dx, nullptr, nullptr, true);
  REQUIRE(out_host && cells_host, "vdn_profiles: null output (out, cells)");
  const int dm = ctx().prm.dm, nscal = ctx().prm.nscal;
  REQUIRE(axis >= 0 && axis < dm, "vdn_profiles: axis = %d is outside 0 .. %d", axis, dm - 1);
  for (int n = 0; n < nlev; n++)
    REQUIRE(mla->pd[n].lo[axis] == mla->pd[0].lo[axis] * (1 << n) && mla->pd[n].hi[axis] - mla->pd[n].lo[axis] + 1 == (mla->pd[0].hi[axis] - mla->pd[0].lo[axis] + 1) << n,
            "vdn_profiles: level %d: the domain is not level 0's refined by %d", n, 1 << n);
  const long want = (long)(mla->pd[0].hi[axis] - mla->pd[0].lo[axis] + 1) << (nlev - 1);
  REQUIRE(nbins == want, "vdn_profiles: nbins = %ld, vdn_profiles_nbins gives %ld", nbins, want);
  vdn_profile_layout lay;
  REQUIRE(layout_of(dm, nscal, &lay), "vdn_profiles: dm = %d, nscal = %d", dm, nscal);
  hipStream_t st = ctx().stream;
  ArenaScope arena;
  const ProfPlan P = profile_plan(nlev, mla->boxes.data(), mla->pd.data(), axis);
  const int nslot = P.slot_start[nlev];
  REQUIRE(nslot > 0, "vdn_profiles: the hierarchy holds no cell");
  const bool wide = nscal > 4;
  const int pq = wide ? (int)PT<PF_MAXS>::PQ : (int)PT<4>::PQ;
  ProfRows R; memset(&R, 0, sizeof R);
  const int nq = wide ? profile_rows<PF_MAXS>(dm, nscal, R) : profile_rows<4>(dm, nscal, R);
  REQUIRE(nq == lay.nrow + 1 && nq <= PF_MAXROW, "vdn_profiles: %d rows, the layout has %d", nq - 1, lay.nrow);
  double *d_part = (double *)arena_alloc(sizeof(double) * (size_t)pq * nslot);
  double *d_out = (double *)arena_alloc(sizeof(double) * (size_t)nq * nbins);          // rows, then the counts
  const bool ranks = comm_active();
  if (ranks) HIPCHK(hipMemsetAsync(d_part, 0, sizeof(double) * (size_t)pq * nslot, st));
  // the tables: ptr and idx of every level, one upload
  ProfTab T; memset(&T, 0, sizeof T); T.nlev = nlev;
  {
    std::vector<int> tab; size_t optr[VDN_MAXLEV], oidx[VDN_MAXLEV];
    for (int n = 0; n < nlev; n++) {
      optr[n] = tab.size(); tab.insert(tab.end(), P.ptr[n].begin(), P.ptr[n].end());
      oidx[n] = tab.size(); tab.insert(tab.end(), P.idx[n].begin(), P.idx[n].end());
    }
    int *d_tab = (int *)arena_alloc(sizeof(int) * tab.size());
    upload_staged(d_tab, tab.data(), sizeof(int) * tab.size());
    for (int n = 0; n < nlev; n++) { T.ptr[n] = d_tab + optr[n]; T.idx[n] = d_tab + oidx[n]; }
  }
  for (int n = 0; n < nlev; n++) {
    const std::vector<int> mine = profile_plan_local(P, n, mla->owner.data(), ctx().rank);
    if (mine.empty()) continue;
    std::vector<CompPiece> pieces(mine.size()); std::vector<int> start(mine.size());
    int nblock = 0;
    for (size_t q = 0; q < mine.size(); q++) {
      const ProfPiece &S = P.pieces[mine[q]];
      pieces[q] = CompPiece{ S.box, { S.lo[0], S.lo[1], S.lo[2] }, { S.hi[0], S.hi[1], S.hi[2] }, S.slot0 };
      start[q] = nblock;
      nblock += axis == 0 ? 1 : S.hi[axis] - S.lo[axis] + 1;
    }
    const CompBox *d_desc = composite_level("vdn_profiles", n, nlev, mla, u, s, pieces);
    int *d_start = (int *)arena_alloc(sizeof(int) * start.size());
    upload_staged(d_start, start.data(), sizeof(int) * start.size());
    const double w = cell_volume(dx, n, dm) / (double)(1 << (nlev - 1 - n));      // a power of two: exact
    if (wide) launch_profile<PF_MAXS>(axis, nblock, d_desc, d_start, (int)pieces.size(), d_part, nscal, dm, w);
    else      launch_profile<4>(axis, nblock, d_desc, d_start, (int)pieces.size(), d_part, nscal, dm, w);
  }
  if (ranks) comm_allreduce_sum_dev(d_part, (size_t)pq * nslot);
  const long nwave = nbins * nq;
  hipLaunchKernelGGL(kk_profile_final, dim3((unsigned)((nwave + PF_THREADS / 64 - 1) / (PF_THREADS / 64))), dim3(PF_THREADS), 0, st, (const double *)d_part, pq, T, R, nq, nbins,
                     d_out, reinterpret_cast<long long *>(d_out + (size_t)lay.nrow * nbins));
  std::vector<double> h((size_t)nq * nbins);
  HIPCHK(hipMemcpyAsync(h.data(), d_out, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  arena.release();
  memcpy(out_host, h.data(), sizeof(double) * (size_t)lay.nrow * nbins);
  memcpy(cells_host, h.data() + (size_t)lay.nrow * nbins, sizeof(long long) * (size_t)nbins);
  VDN_CATCH
}
