// pdf.hip -- how much of the fluid has which value: vdn_pdf, vdn_pdf2, vdn_pdf_layout (include/varden_amd.h).  Volume-weighted distributions and conditional sums
// of a hierarchy's fields over the COMPOSITE grid of vdn_diagnostics, binned by VALUE on a uniform axis.  No reference counterpart; DESIGN.md section 23.
//
// Definition.  The bin field q of a cell is s(comp), u(comp), magvel_value or vort_value (derived.h); its slot on the axis {lo, hi, nbins} is pdf_slot (pdf_bin.h):
// nbins + 2 slots, "below", the bins, "above"; a NaN q counts in nan_cells alone.  Per slot: the exact number of composite cells of every level, and the sums of
// q dV, s_c dV, u_d dV, (rho u_d) dV and ((0.5 rho) (u.u)) dV over the slot's cells, dV the cell volume of the cell's level.  volume is formed on the host from the
// counts: sum over the levels, ascending, of cells[l][slot] * dV_l.
//
// Launch form.  The slab cut of diag_plan.h, unchanged: one launch per level (kk_pdf), a workgroup of four waves per slab, the thread -> cell map of composite.h -- cell
// t + 256 e of a trip, (i, j, k) stepped by constants with one carry each --, the loads of the UNR cells of a trip issued before the first is used.
//   counts   the destination of a cell depends on its value, so a thread cannot keep a register per slot.  Integer atomics into 32-bit LDS counters (a slab holds
//            at most 64 K cells), flushed with 64-bit integer atomics into a (level, slot) table in memory.  Integer addition is exact in any order.  Between ranks
//            the table travels as integers held in doubles (exact below 2^53), as the cells row of vdn_profiles does.
//   sums     no floating-point atomic, in LDS or in memory.  Each wave owns one LDS copy of the (slot, row) table.  In every trip, for each of its UNR cells in
//            turn, the wave loops over the DISTINCT slots among its lanes: it takes the slot of the first remaining lane, ballots the lanes that share it, sums every
//            row over the whole wave through the fixed shuffle tree -- the other lanes contribute +0.0 --, adds the result to its LDS entry from lane 0 and retires
//            those lanes.  Covered cells, the lanes past the slab's end and NaN-q cells take no part.  A wave's entry therefore depends on the slab alone: fixed map,
//            cells in order, trips in order, fixed tree.  The four waves meet as (w0 + w1) + (w2 + w3), and ONE partial per (slab, slot, row) goes to the slab's place
//            in an array indexed by the GLOBAL slab number.  Several ranks: the places of foreign slabs are zero and one sum all-reduce fills them (x + 0 + ... + 0
//            is x).  kk_pdf_final then gives a wave to every (slot, row): starting from +0 it adds the slabs in slab order (slot_sum of composite.h).  The bits of
//            a result depend on the box lists and the fields alone -- not on the call, the rank or the number of ranks; composite.h states what that rests on.
// LDS budget (dynamic, sized by the call): 4 wave copies x (nbins + 2) slots x nr rows x 8 B, nr = nscal + 2 dm + 2 (every row but volume), plus 4 (nbins + 3) B of
// counters.  64 bins, nscal = 2, dm = 3: 21 KB.  256 bins: 258 x 10 x 8 = 20.2 KB a copy, 82 KB in all, at nscal = 2; 258 x 19 x 8 = 38.3 KB a copy, 153.2 KB in all
// (157,900 B with the counters), at nscal = 11 -- under the 160 KB (163,840 B) a workgroup of a gfx950 CU may hold, so every case keeps four copies and one tree.
// More than 64 KB needs hipFuncAttributeMaxDynamicSharedMemorySize, set once per instantiation.  One workgroup per CU is then resident; a slab per CU is what the
// plan gives a 256^3 box anyway.
// vdn_pdf2 is the same march with two slot computations and a (n1 + 2) x (n2 + 2) table of 32-bit LDS counters (66 x 66 at most: 17 KB, static); counts only.
// Memory: descriptors, partials, counters, the covered-cell masks and the result live in the arena of the call's ArenaScope;
// one copy brings the result home.  The calls write none of their inputs; only VDN_PDF_VORTICITY reads a ghost cell (one layer of u).
#include "composite.h"
#include "pdf_bin.h"
#include <atomic>

namespace {
constexpr int PD_THREADS = COMP_THREADS, PD_WAVES = COMP_WAVES, PD_MAXS = 11;
constexpr size_t PD_LDS_MAX = 160 * 1024, PD_LDS_PLAIN = 64 * 1024;
static_assert(VDN_PDF_MAX_BINS + 2 <= 65536 && DIAG_SLAB_CELLS <= 0xffffffffl, "a slab's count fits a 32-bit counter");

struct PdfAx { int field, comp, nbins; double lo, hi, w; };

template <bool VORT>
DEVI double pdf_q(const PdfAx &X, const FV &fu, const FV &fs, const VortArgs &A, int dm, int i, int j, int k) {
  if (X.field == VDN_PDF_SCALAR) return fv_get(fs, i, j, k, X.comp);
  if (X.field == VDN_PDF_VELOCITY) return fv_get(fu, i, j, k, X.comp);
  if (X.field == VDN_PDF_MAGVEL) return magvel_value(fu, dm, i, j, k);
  if constexpr (VORT) return vort_value(fu, A, i, j, k);
  return 0.0;
}

// NS: the scalars the instantiation can carry (nscal <= NS; the loops over them are unrolled so that every term is a register); VORT: q may be the vorticity.
// The rows of a thread's terms: q, s[NS], u[3], ru[3], ke; row j of them lives at column pd_col(j) of the LDS table, whose nr = nscal + 2 dm + 2 columns are the
// rows 1 .. nrow-1 of vdn_pdf_layout in order (-1: the row does not exist for this nscal / dm).
template <int NS> DEVI int pd_col(int j, int nscal, int dm) {
  if (j == 0) return 0;
  if (j < 1 + NS) return j - 1 < nscal ? j : -1;
  if (j < 4 + NS) return j - 1 - NS < dm ? 1 + nscal + (j - 1 - NS) : -1;
  if (j < 7 + NS) return j - 4 - NS < dm ? 1 + nscal + dm + (j - 4 - NS) : -1;
  return 1 + nscal + 2 * dm;
}
template <int NS, bool VORT>
__global__ void __launch_bounds__(PD_THREADS) kk_pdf(const CompBoxV *descs, PdfAx X, double *__restrict__ part, u64 *__restrict__ gcnt, u64 *__restrict__ gnan,
                                                     int nscal, int dm, double vol) {
  extern __shared__ double pd_lds[];
  constexpr int NRT = NS + 8, UNR = NS <= 4 ? 4 : 2;
  const CompBoxV &D = as_constant(descs + blockIdx.x);
  const int nslot = X.nbins + 2, nr = nscal + 2 * dm + 2, ne = nslot * nr;
  const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
  double *mine = pd_lds + (long)wave * ne;                                   // this wave's copy of the (slot, row) table
  unsigned *cnt = reinterpret_cast<unsigned *>(pd_lds + (long)PD_WAVES * ne);     // [nslot], then the NaN cells
  for (int e = t; e < PD_WAVES * ne; e += PD_THREADS) pd_lds[e] = 0.0;
  for (int e = t; e <= nslot; e += PD_THREADS) cnt[e] = 0u;
  __syncthreads();
  const int nx = D.hi[0] - D.lo[0] + 1, ny = D.hi[1] - D.lo[1] + 1, nz = D.hi[2] - D.lo[2] + 1;
  const int tot = nx * ny * nz;
  const unsigned char *mask = D.mask;
  const FV fu = D.u, fs = D.s;
  CellMap M(nx, ny, t);
  int nnan = 0;
  // the trip loop is wave-uniform (it runs on the wave's first cell), so that every lane takes part in every ballot and shuffle; a lane past the slab's end loads
  // the slab's first cell and is dropped, as a covered cell is
  for (int t0 = t - lane; t0 < tot; t0 += UNR * PD_THREADS) {
    double uv[UNR][3], sv[UNR][NS], wv[UNR];
    bool live[UNR];
    #pragma unroll
    for (int e = 0; e < UNR; e++) {
      live[e] = t0 + lane + e * PD_THREADS < tot;
      const int i = D.lo[0] + (live[e] ? M.ci : 0), j = D.lo[1] + (live[e] ? M.cj : 0), k = D.lo[2] + (live[e] ? M.ck : 0);
      M.step();
      live[e] = load_cell<NS>(D, fu, fs, mask, i, j, k, live[e], nscal, dm, uv[e], sv[e]);
      wv[e] = 0.0;
      if constexpr (VORT) { if (X.field == VDN_PDF_VORTICITY) wv[e] = vort_value(fu, D.A, i, j, k); }
    }
    #pragma unroll
    for (int e = 0; e < UNR; e++) {
      double q2 = uv[e][0] * uv[e][0] + uv[e][1] * uv[e][1];                  // magvel_value's expression (derived.h), on the values already loaded
      if (dm == 3) q2 = q2 + uv[e][2] * uv[e][2];
      // q from the registers: the field is the same for the whole launch, the component is picked by compares (no indexed register)
      double q = wv[e];
      if (X.field == VDN_PDF_SCALAR) {
        q = sv[e][0];
        #pragma unroll
        for (int c = 1; c < NS; c++) q = c == X.comp ? sv[e][c] : q;
      } else if (X.field == VDN_PDF_VELOCITY) {
        q = X.comp == 0 ? uv[e][0] : X.comp == 1 ? uv[e][1] : uv[e][2];
      } else if (X.field == VDN_PDF_MAGVEL) {
        q = sqrt(q2);
      }
      const int slot = live[e] ? pdf_slot(q, X.lo, X.hi, X.w, X.nbins) : PDF_NO_SLOT;
      if (live[e] && slot == PDF_NO_SLOT) nnan++;
      const bool in = slot != PDF_NO_SLOT;
      if (in) atomicAdd(&cnt[slot], 1u);
      // the terms: products associated as include/varden_amd.h writes them, then the cell volume
      double r[NRT];
      r[0] = q * vol;
      #pragma unroll
      for (int c = 0; c < NS; c++) r[1 + c] = sv[e][c] * vol;
      #pragma unroll
      for (int d = 0; d < 3; d++) { r[1 + NS + d] = uv[e][d] * vol; r[4 + NS + d] = (sv[e][0] * uv[e][d]) * vol; }
      r[7 + NS] = ((0.5 * sv[e][0]) * q2) * vol;
      // the distinct slots among the wave's lanes, in the order of their first lanes
      u64 rem = __ballot(in);
      while (rem) {
        const int sl = __shfl(slot, __ffsll((long long)rem) - 1, 64);
        const bool member = in && slot == sl;
        // every row's tree first, the LDS adds afterwards: the trees are independent and their shuffles may overlap (tree by tree, with the add and its branch in
        // between, a trip waits for one shuffle after the other: 5.6 ms against 3.6 ms per density call on a 256^3 box); the operations,
        // and with them the bits, are the same
        double v[NRT];
        #pragma unroll
        for (int j = 0; j < NRT; j++) v[j] = wave_sum(member ? r[j] : 0.0);      // (rows beyond nscal / dm too: zeros, and no branch between the trees)
        if (lane == 0) {
          #pragma unroll
          for (int j = 0; j < NRT; j++) {
            const int col = pd_col<NS>(j, nscal, dm);
            if (col >= 0) mine[sl * nr + col] = mine[sl * nr + col] + v[j];
          }
        }
        rem &= ~__ballot(member);
      }
    }
  }
  if (nnan) atomicAdd(&cnt[nslot], (unsigned)nnan);
  __syncthreads();
  // the four waves: (w0 + w1) + (w2 + w3), one partial per (slot, row) into the slab's place; the counters into the level's table
  double *out = part + (long)D.slot * ne;
  for (int e = t; e < ne; e += PD_THREADS) out[e] = sum4(pd_lds[e], pd_lds[ne + e], pd_lds[2 * ne + e], pd_lds[3 * ne + e]);
  for (int e = t; e <= nslot; e += PD_THREADS) {
    const unsigned c = cnt[e];
    if (c) atomicAdd(e < nslot ? gcnt + e : gnan, (u64)c);
  }
}

// a wave per (slot, row): starting from +0, the slabs in slab order
__global__ void __launch_bounds__(PD_THREADS) kk_pdf_final(const double *__restrict__ part, int ne, int nslab, double *__restrict__ out) {
  const int g = (int)blockIdx.x * PD_WAVES + ((int)threadIdx.x >> 6), lane = (int)threadIdx.x & 63;
  if (g >= ne) return;
  const double v = slot_sum(0.0, part, ne, g, nullptr, 0, nslab, lane);
  if (lane == 0) out[g] = v;
}
// the 64-bit counters as doubles (exact: a hierarchy holds far fewer than 2^53 cells), the form the all-reduce and the copy home take
__global__ void kk_pdf_counts(const u64 *__restrict__ cnt, int n, double *__restrict__ out) {
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i < n) out[i] = (double)cnt[i];
}

constexpr int PD2_SIDE = VDN_PDF2_MAX_BINS + 2;
template <bool VORT>
__global__ void __launch_bounds__(PD_THREADS) kk_pdf2(const CompBoxV *descs, PdfAx X1, PdfAx X2, u64 *__restrict__ gcnt, u64 *__restrict__ gnan, int dm) {
  __shared__ unsigned cnt[PD2_SIDE * PD2_SIDE + 1];                          // [n1 + 2][n2 + 2], then the NaN cells
  constexpr int UNR = 4;
  const CompBoxV &D = as_constant(descs + blockIdx.x);
  const int t = (int)threadIdx.x, n2 = X2.nbins + 2, ne = (X1.nbins + 2) * n2;
  for (int e = t; e <= ne; e += PD_THREADS) cnt[e] = 0u;
  __syncthreads();
  const int nx = D.hi[0] - D.lo[0] + 1, ny = D.hi[1] - D.lo[1] + 1, nz = D.hi[2] - D.lo[2] + 1;
  const int tot = nx * ny * nz;
  const unsigned char *mask = D.mask;
  const FV fu = D.u, fs = D.s;
  CellMap M(nx, ny, t);
  int nnan = 0;
  for (int t0 = t; t0 < tot; t0 += UNR * PD_THREADS) {
    double q1[UNR], q2[UNR];
    bool live[UNR];
    #pragma unroll
    for (int e = 0; e < UNR; e++) {
      live[e] = t0 + e * PD_THREADS < tot;
      const int i = D.lo[0] + (live[e] ? M.ci : 0), j = D.lo[1] + (live[e] ? M.cj : 0), k = D.lo[2] + (live[e] ? M.ck : 0);
      M.step();
      live[e] = live[e] && cell_open(D, mask, i, j, k);
      q1[e] = pdf_q<VORT>(X1, fu, fs, D.A, dm, i, j, k);
      q2[e] = pdf_q<VORT>(X2, fu, fs, D.A, dm, i, j, k);
    }
    #pragma unroll
    for (int e = 0; e < UNR; e++) {
      if (!live[e]) continue;
      const int s1 = pdf_slot(q1[e], X1.lo, X1.hi, X1.w, X1.nbins), s2 = pdf_slot(q2[e], X2.lo, X2.hi, X2.w, X2.nbins);
      if (s1 == PDF_NO_SLOT || s2 == PDF_NO_SLOT) nnan++;
      else atomicAdd(&cnt[s1 * n2 + s2], 1u);
    }
  }
  if (nnan) atomicAdd(&cnt[ne], (unsigned)nnan);
  __syncthreads();
  for (int e = t; e <= ne; e += PD_THREADS) {
    const unsigned c = cnt[e];
    if (c) atomicAdd(e < ne ? gcnt + e : gnan, (u64)c);
  }
}

// more than 64 KB of dynamic LDS: the function attribute, once per instantiation
template <int NS, bool VORT> void launch_pdf(int nd, size_t lds, const CompBoxV *d, const PdfAx &X, double *part, u64 *gcnt, u64 *gnan, int nscal, int dm, double vol) {
  static std::atomic<bool> raised{ false };
  if (lds > PD_LDS_PLAIN && !raised.load()) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&kk_pdf<NS, VORT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)PD_LDS_MAX));
    raised.store(true);
  }
  hipLaunchKernelGGL((kk_pdf<NS, VORT>), dim3(nd), dim3(PD_THREADS), lds, ctx().stream, d, X, part, gcnt, gnan, nscal, dm, vol);
}

bool layout_of(int dm, int nscal, vdn_pdf_layout_t *lay) {
  if (!lay || (dm != 2 && dm != 3) || nscal < 1 || nscal > PD_MAXS) return false;
  lay->volume = 0; lay->q = 1; lay->s = 2; lay->u = lay->s + nscal; lay->ru = lay->u + dm; lay->ke = lay->ru + dm; lay->nrow = lay->ke + 1;
  return true;
}

PdfAx check_axis(const char *name, const char *which, int field, int comp, int nbins, double lo, double hi, int maxbins) {
  const int dm = ctx().prm.dm, nscal = ctx().prm.nscal;
  REQUIRE(field >= VDN_PDF_SCALAR && field <= VDN_PDF_VORTICITY, "%s: %sfield = %d is not a VDN_PDF_ code (0 .. 3)", name, which, field);
  REQUIRE(field != VDN_PDF_SCALAR || (comp >= 0 && comp < nscal), "%s: %scomp = %d is outside 0 .. %d (nscal = %d)", name, which, comp, nscal - 1, nscal);
  REQUIRE(field != VDN_PDF_VELOCITY || (comp >= 0 && comp < dm), "%s: %scomp = %d is outside 0 .. %d (dm = %d)", name, which, comp, dm - 1, dm);
  REQUIRE(nbins >= 1 && nbins <= maxbins, "%s: %snbins = %d is outside 1 .. %d", name, which, nbins, maxbins);
  REQUIRE(fabs(lo) < __builtin_huge_val() && fabs(hi) < __builtin_huge_val() && lo < hi, "%s: %srange: lo = %g and hi = %g must be finite with lo < hi", name, which, lo, hi);
  PdfAx X; X.field = field; X.comp = comp; X.nbins = nbins; X.lo = lo; X.hi = hi; X.w = pdf_width(lo, hi, nbins);
  REQUIRE(X.w > 0.0 && X.w < __builtin_huge_val(), "%s: %srange: the bin width (hi - lo) / nbins = %g is not a positive finite number", name, which, X.w);
  return X;
}

}   // namespace

extern "C" size_t vdn_pdf_layout_sizeof(void) { return sizeof(vdn_pdf_layout_t); }

extern "C" int vdn_pdf_layout(int dm, int nscal, vdn_pdf_layout_t *lay) {
  if (layout_of(dm, nscal, lay)) return 0;
  vdn_set_error("vdn_pdf_layout: dm = %d (2 or 3), nscal = %d (1 .. %d), lay %s", dm, nscal, PD_MAXS, lay ? "given" : "NULL");
  return 1;
}

extern "C" int vdn_pdf(int nlev, vdn_layout *mla, vdn_multifab *const *u, vdn_multifab *const *s, const double *dx, const vdn_bc_tower *bct,
                       int field, int comp, int nbins, double lo, double hi, double *out_host, long long *cells_host, long long *nan_cells) {
  VDN_TRY
  const bool vort = field == VDN_PDF_VORTICITY;
  composite_check("vdn_pdf", nlev, mla, u, s, dx, bct, vort ? "VDN_PDF_VORTICITY" : nullptr, true);
  REQUIRE(out_host && cells_host && nan_cells, "vdn_pdf: null output (out, cells, nan_cells)");
  const PdfAx X = check_axis("vdn_pdf", "", field, comp, nbins, lo, hi, VDN_PDF_MAX_BINS);
  const int dm = ctx().prm.dm, nscal = ctx().prm.nscal;
  vdn_pdf_layout_t lay;
  REQUIRE(layout_of(dm, nscal, &lay), "vdn_pdf: dm = %d, nscal = %d", dm, nscal);
  const int nslot = nbins + 2, nr = lay.nrow - 1, ne = nslot * nr;
  const size_t lds = sizeof(double) * (size_t)PD_WAVES * ne + sizeof(unsigned) * (size_t)(nslot + 1);
  REQUIRE(lds <= PD_LDS_MAX, "vdn_pdf: %zu bytes of LDS wanted, a workgroup holds %zu", lds, PD_LDS_MAX);
  hipStream_t st = ctx().stream;
  ArenaScope arena;
  int lev_start[VDN_MAXLEV + 1];
  const std::vector<DiagSlab> slabs = diag_plan(nlev, mla->boxes.data(), lev_start);
  const int nslab = lev_start[nlev];
  REQUIRE(nslab > 0, "vdn_pdf: the hierarchy holds no cell");
  // one array of doubles: the partials [nslab][slot][row], the counts [nlev][slot] and the NaN cells, the sums [slot][row]
  const int ncnt = nlev * nslot + 1;
  const size_t npart = (size_t)nslab * ne;
  double *d_part = (double *)arena_alloc(sizeof(double) * (npart + ncnt + ne));
  double *d_cntd = d_part + npart, *d_out = d_cntd + ncnt;
  u64 *d_cnt = (u64 *)arena_alloc(sizeof(u64) * ncnt);
  HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(u64) * ncnt, st));
  const bool ranks = comm_active();
  if (ranks) HIPCHK(hipMemsetAsync(d_part, 0, sizeof(double) * npart, st));
  double vol[VDN_MAXLEV];
  for (int n = 0; n < nlev; n++) {
    vol[n] = cell_volume(dx, n, dm);
    const std::vector<CompPiece> mine = slab_pieces(slabs, n, mla);
    if (mine.empty()) continue;
    const CompBoxV *d_desc = composite_level_vort("vdn_pdf", n, nlev, mla, u, s, mine, dx, bct, vort);
    const int nd = (int)mine.size();
    u64 *gc = d_cnt + (size_t)n * nslot, *gn = d_cnt + (size_t)nlev * nslot;
    if (nscal <= 4) { if (vort) launch_pdf<4, true>(nd, lds, d_desc, X, d_part, gc, gn, nscal, dm, vol[n]); else launch_pdf<4, false>(nd, lds, d_desc, X, d_part, gc, gn, nscal, dm, vol[n]); }
    else            { if (vort) launch_pdf<PD_MAXS, true>(nd, lds, d_desc, X, d_part, gc, gn, nscal, dm, vol[n]); else launch_pdf<PD_MAXS, false>(nd, lds, d_desc, X, d_part, gc, gn, nscal, dm, vol[n]); }
  }
  hipLaunchKernelGGL(kk_pdf_counts, dim3((ncnt + 255) / 256), dim3(256), 0, st, (const u64 *)d_cnt, ncnt, d_cntd);
  if (ranks) comm_allreduce_sum_dev(d_part, npart + ncnt);
  hipLaunchKernelGGL(kk_pdf_final, dim3((ne + PD_WAVES - 1) / PD_WAVES), dim3(PD_THREADS), 0, st, (const double *)d_part, ne, nslab, d_out);
  std::vector<double> h((size_t)ncnt + ne);
  HIPCHK(hipMemcpyAsync(h.data(), d_cntd, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  arena.release();
  for (int n = 0; n < VDN_MAXLEV; n++)
    for (int m = 0; m < nslot; m++) cells_host[(size_t)n * nslot + m] = n < nlev ? (long long)h[(size_t)n * nslot + m] : 0;
  *nan_cells = (long long)h[(size_t)nlev * nslot];
  for (int m = 0; m < nslot; m++) {
    double v = 0.0;
    for (int n = 0; n < nlev; n++) v = v + (double)cells_host[(size_t)n * nslot + m] * vol[n];
    out_host[(size_t)lay.volume * nslot + m] = v;
    for (int r = 0; r < nr; r++) out_host[(size_t)(r + 1) * nslot + m] = h[(size_t)ncnt + (size_t)m * nr + r];
  }
  VDN_CATCH
}

extern "C" int vdn_pdf2(int nlev, vdn_layout *mla, vdn_multifab *const *u, vdn_multifab *const *s, const double *dx, const vdn_bc_tower *bct,
                        int field1, int comp1, int nbins1, double lo1, double hi1, int field2, int comp2, int nbins2, double lo2, double hi2,
                        long long *cells_host, double *volume_host, long long *nan_cells) {
  VDN_TRY
  const bool vort = field1 == VDN_PDF_VORTICITY || field2 == VDN_PDF_VORTICITY;
  composite_check("vdn_pdf2", nlev, mla, u, s, dx, bct, vort ? "VDN_PDF_VORTICITY" : nullptr, true);
  REQUIRE(cells_host && volume_host && nan_cells, "vdn_pdf2: null output (cells, volume, nan_cells)");
  const PdfAx X1 = check_axis("vdn_pdf2", "axis 1: ", field1, comp1, nbins1, lo1, hi1, VDN_PDF2_MAX_BINS);
  const PdfAx X2 = check_axis("vdn_pdf2", "axis 2: ", field2, comp2, nbins2, lo2, hi2, VDN_PDF2_MAX_BINS);
  const int dm = ctx().prm.dm;
  const int ne = (nbins1 + 2) * (nbins2 + 2), ncnt = nlev * ne + 1;
  hipStream_t st = ctx().stream;
  ArenaScope arena;
  int lev_start[VDN_MAXLEV + 1];
  const std::vector<DiagSlab> slabs = diag_plan(nlev, mla->boxes.data(), lev_start);
  REQUIRE(lev_start[nlev] > 0, "vdn_pdf2: the hierarchy holds no cell");
  double *d_cntd = (double *)arena_alloc(sizeof(double) * ncnt);
  u64 *d_cnt = (u64 *)arena_alloc(sizeof(u64) * ncnt);
  HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(u64) * ncnt, st));
  double vol[VDN_MAXLEV];
  for (int n = 0; n < nlev; n++) {
    vol[n] = cell_volume(dx, n, dm);
    const std::vector<CompPiece> mine = slab_pieces(slabs, n, mla);
    if (mine.empty()) continue;
    const CompBoxV *d_desc = composite_level_vort("vdn_pdf2", n, nlev, mla, u, s, mine, dx, bct, vort);
    const int nd = (int)mine.size();
    u64 *gc = d_cnt + (size_t)n * ne, *gn = d_cnt + (size_t)nlev * ne;
    if (vort) hipLaunchKernelGGL((kk_pdf2<true>), dim3(nd), dim3(PD_THREADS), 0, st, d_desc, X1, X2, gc, gn, dm);
    else      hipLaunchKernelGGL((kk_pdf2<false>), dim3(nd), dim3(PD_THREADS), 0, st, d_desc, X1, X2, gc, gn, dm);
  }
  hipLaunchKernelGGL(kk_pdf_counts, dim3((ncnt + 255) / 256), dim3(256), 0, st, (const u64 *)d_cnt, ncnt, d_cntd);
  if (comm_active()) comm_allreduce_sum_dev(d_cntd, (size_t)ncnt);
  std::vector<double> h((size_t)ncnt);
  HIPCHK(hipMemcpyAsync(h.data(), d_cntd, sizeof(double) * h.size(), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  arena.release();
  for (int n = 0; n < VDN_MAXLEV; n++)
    for (int m = 0; m < ne; m++) cells_host[(size_t)n * ne + m] = n < nlev ? (long long)h[(size_t)n * ne + m] : 0;
  *nan_cells = (long long)h[(size_t)nlev * ne];
  for (int m = 0; m < ne; m++) {
    double v = 0.0;
    for (int n = 0; n < nlev; n++) v = v + (double)cells_host[(size_t)n * ne + m] * vol[n];
    volume_host[m] = v;
  }
  VDN_CATCH
}
