// composite.hip -- the host side of composite.h: what vdn_diagnostics, vdn_profiles, vdn_pdf and vdn_pdf2 ask of their arguments, the byte masks of the cells
// a finer level covers, and the descriptors of a level's local pieces.  Everything here lives in the caller's ArenaScope.
#include "composite.h"

void composite_check(const char *name, int nlev, const vdn_layout *mla, vdn_multifab *const *u, vdn_multifab *const *s, const double *dx, const vdn_bc_tower *bct,
                     const char *vort, bool ratio2) {
  REQUIRE(ctx().inited, "%s: vdn_init has not been called", name);
  REQUIRE(mla && u && s, "%s: null argument (mla, u, s)", name);
  REQUIRE(nlev >= 1 && nlev <= VDN_MAXLEV, "%s: nlev = %d is outside 1 .. %d", name, nlev, VDN_MAXLEV);
  REQUIRE(nlev == mla->nlev, "%s: nlev = %d does not match the layout's %d levels", name, nlev, mla->nlev);
  const int dm = ctx().prm.dm, nscal = ctx().prm.nscal;
  REQUIRE(dm == 3 || nlev == 1, "%s: dm = 2 runs on one level (nlev = %d)", name, nlev);
  REQUIRE(dx, "%s: dx is NULL (every cell is weighted by its volume)", name);
  REQUIRE(!vort || bct, "%s: %s needs the bc tower (bct is NULL)", name, vort);
  for (int n = 0; n < nlev; n++) {
    REQUIRE(u[n] && s[n], "%s: level %d: null multifab", name, n);
    REQUIRE(u[n]->la == mla && s[n]->la == mla && u[n]->lev == n && s[n]->lev == n, "%s: level %d: the layouts of u and s differ (from each other or from mla)", name, n);
    REQUIRE(u[n]->nfabs() == s[n]->nfabs(), "%s: level %d: the layouts of u and s differ (%d and %d local boxes)", name, n, u[n]->nfabs(), s[n]->nfabs());
    REQUIRE(u[n]->nc >= dm && s[n]->nc >= nscal, "%s: level %d: u carries %d components (dm = %d), s %d (nscal = %d)", name, n, u[n]->nc, dm, s[n]->nc, nscal);
    for (int d = 0; d < 3; d++) REQUIRE(!u[n]->nodal[d] && !s[n]->nodal[d], "%s: level %d: cell-centred multifabs expected", name, n);
    REQUIRE(!vort || u[n]->ng >= 1, "%s: level %d: %s reads one ghost layer of u (ng = %d)", name, n, vort, u[n]->ng);
    if (ratio2 && n < nlev - 1) for (int d = 0; d < 3; d++) REQUIRE(mla->rr[3 * n + d] == 2, "%s: level %d: a refinement ratio of 2 is expected (it is %d along %d)", name, n, mla->rr[3 * n + d], d);
  }
}

double cell_volume(const double *dx, int n, int dm) {
  double vol = dx[3 * n] * dx[3 * n + 1];
  if (dm == 3) vol = vol * dx[3 * n + 2];
  return vol;
}

std::vector<CompPiece> slab_pieces(const std::vector<DiagSlab> &slabs, int n, const vdn_layout *mla) {
  std::vector<CompPiece> out;
  for (int q : diag_plan_local(slabs, n, mla->owner.data(), ctx().rank)) {
    const vdn_box &B = mla->boxes[n][slabs[q].box];
    out.push_back(CompPiece{ slabs[q].box, { B.lo[0], B.lo[1], slabs[q].k0 }, { B.hi[0], B.hi[1], slabs[q].k1 }, q });
  }
  return out;
}

namespace {
// the cells of a level that the next level covers: a byte per valid cell of every local box, set box pair by box pair (the box-batched cell launch of vdn_dev.h)
struct cover_K { unsigned char *m; int blo[3], bnx, bny;
  __device__ void cell(int i, int j, int k) const { m[((long)(k - blo[2]) * bny + (j - blo[1])) * bnx + (i - blo[0])] = 1; } };
// the mask of every local box of level n of `mf` (arena memory)
std::vector<unsigned char *> cover_masks(const vdn_layout *la, const vdn_multifab *mf, int n) {
  hipStream_t st = ctx().stream;
  const int nb = mf->nfabs();
  std::vector<unsigned char *> m(nb, nullptr);
  if (nb == 0) return m;
  size_t total = 0; std::vector<size_t> off(nb);
  for (int b = 0; b < nb; b++) {
    off[b] = total;
    size_t c = 1; for (int d = 0; d < 3; d++) c *= (size_t)(mf->vbox[b].hi[d] - mf->vbox[b].lo[d] + 1);
    total += (c + 63) & ~(size_t)63;
  }
  unsigned char *base = (unsigned char *)arena_alloc(total);
  HIPCHK(hipMemsetAsync(base, 0, total, st));
  for (int b = 0; b < nb; b++) m[b] = base + off[b];
  std::vector<std::pair<cover_K, Range3>> v;
  const BoxBins bins(mf->vbox);
  for (const vdn_box &f : la->boxes[n + 1]) {
    int clo[3], chi[3];
    for (int d = 0; d < 3; d++) { const int r = la->rr[3 * n + d]; clo[d] = f.lo[d] / r; chi[d] = f.hi[d] / r; }
    for (int b : bins.near(clo, chi, 0)) {
      cover_K q; Range3 r; bool any = true;
      for (int d = 0; d < 3; d++) { r.lo[d] = std::max(clo[d], mf->vbox[b].lo[d]); r.hi[d] = std::min(chi[d], mf->vbox[b].hi[d]); any = any && r.lo[d] <= r.hi[d]; q.blo[d] = mf->vbox[b].lo[d]; }
      if (!any) continue;
      q.m = m[b]; q.bnx = mf->vbox[b].hi[0] - mf->vbox[b].lo[0] + 1; q.bny = mf->vbox[b].hi[1] - mf->vbox[b].lo[1] + 1;
      v.push_back({ q, r });
    }
  }
  launch_cells(v, st);
  return m;
}

// D: CompBox, or CompBoxV with the arguments of vort_value
template <class D>
const D *level_boxes(const char *name, int n, int nlev, const vdn_layout *mla, vdn_multifab *const *u, vdn_multifab *const *s, const std::vector<CompPiece> &pieces,
                     const double *dx, const vdn_bc_tower *bct, bool vort) {
  std::vector<int> local_of(mla->boxes[n].size(), -1);          // global box -> local index
  for (int i = 0; i < (int)mla->local[n].size(); i++) local_of[mla->local[n][i]] = i;
  std::vector<unsigned char *> mask;
  if (n < nlev - 1) mask = cover_masks(mla, u[n], n);
  std::vector<D> v(pieces.size());
  for (size_t q = 0; q < pieces.size(); q++) {
    const CompPiece &S = pieces[q];
    const int b = S.box >= 0 && S.box < (int)local_of.size() ? local_of[S.box] : -1;
    REQUIRE(b >= 0 && b < u[n]->nfabs(), "%s: level %d: box %d is not local", name, n, S.box);
    const vdn_box &B = u[n]->vbox[b];
    D &C = v[q];
    C.u = u[n]->fabs[b]; C.s = s[n]->fabs[b]; C.mask = mask.empty() ? nullptr : mask[b]; C.slot = S.slot;
    for (int d = 0; d < 3; d++) {
      REQUIRE(B.lo[d] == s[n]->vbox[b].lo[d] && B.hi[d] == s[n]->vbox[b].hi[d], "%s: level %d: the layouts of u and s differ", name, n);
      REQUIRE(S.lo[d] >= B.lo[d] && S.hi[d] <= B.hi[d] && S.lo[d] <= S.hi[d], "%s: level %d: box %d differs between the layout and the multifab", name, n, S.box);
      C.blo[d] = B.lo[d]; C.lo[d] = S.lo[d]; C.hi[d] = S.hi[d];
    }
    C.bnx = B.hi[0] - B.lo[0] + 1; C.bny = B.hi[1] - B.lo[1] + 1;
    if constexpr (std::is_same<D, CompBoxV>::value) {
      const int dm = ctx().prm.dm;
      if (vort) C.A = vort_args(u[n], b, bct, dx + 3 * n, dm, 0); else { C.A = VortArgs(); C.A.dm = dm; }
    }
  }
  D *d_desc = (D *)arena_alloc(sizeof(D) * v.size());
  upload_staged(d_desc, v.data(), sizeof(D) * v.size());
  return d_desc;
}
}   // namespace

const CompBox *composite_level(const char *name, int n, int nlev, const vdn_layout *mla, vdn_multifab *const *u, vdn_multifab *const *s, const std::vector<CompPiece> &pieces) {
  return level_boxes<CompBox>(name, n, nlev, mla, u, s, pieces, nullptr, nullptr, false);
}
const CompBoxV *composite_level_vort(const char *name, int n, int nlev, const vdn_layout *mla, vdn_multifab *const *u, vdn_multifab *const *s, const std::vector<CompPiece> &pieces,
                                     const double *dx, const vdn_bc_tower *bct, bool vort) {
  return level_boxes<CompBoxV>(name, n, nlev, mla, u, s, pieces, dx, bct, vort);
}
