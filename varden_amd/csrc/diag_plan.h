// diag_plan.h -- the slab split of vdn_diagnostics (diag.hip), host only: no HIP, no library type, so tests/cpp/diag_plan_check.cpp holds it without a GPU.
//
// A slab is a run of whole k-planes of one box, about DIAG_SLAB_CELLS cells; one workgroup reduces one slab to one partial per quantity.  The slabs of a
// hierarchy are numbered in (level, global box index, k) order from the GLOBAL box lists alone: the number of a slab -- the slot of its partials -- does
// not depend on which rank owns its box, and the final sum runs over the slots in that order on every rank.
#pragma once
#include <vector>

constexpr long DIAG_SLAB_CELLS = 65536;
struct DiagSlab { int lev, box, k0, k1; };        // box: the global index on its level; planes k0 .. k1, both included

// planes per slab of a box: whole planes, at most DIAG_SLAB_CELLS cells (one plane when a plane alone is larger), spread evenly over the slabs
inline int diag_slab_planes(const int lo[3], const int hi[3]) {
  const long plane = (long)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1);
  const int nz = hi[2] - lo[2] + 1;
  long kper = DIAG_SLAB_CELLS / (plane > 0 ? plane : 1);
  if (kper < 1) kper = 1;
  if (kper > nz) kper = nz;
  const int nslab = (int)((nz + kper - 1) / kper);
  return (nz + nslab - 1) / nslab;
}
// every slab of levels 0 .. nlev-1; B: anything with int lo[3], hi[3].  lev_start[n] = the number of level n's first slab, lev_start[nlev] = their count
template <class B>
inline std::vector<DiagSlab> diag_plan(int nlev, const std::vector<B> *boxes, int *lev_start) {
  std::vector<DiagSlab> out;
  for (int n = 0; n < nlev; n++) {
    lev_start[n] = (int)out.size();
    for (int b = 0; b < (int)boxes[n].size(); b++) {
      const B &q = boxes[n][b];
      if (q.hi[0] < q.lo[0] || q.hi[1] < q.lo[1] || q.hi[2] < q.lo[2]) continue;
      const int kper = diag_slab_planes(q.lo, q.hi);
      for (int k = q.lo[2]; k <= q.hi[2]; k += kper) out.push_back(DiagSlab{ n, b, k, k + kper - 1 < q.hi[2] ? k + kper - 1 : q.hi[2] });
    }
  }
  lev_start[nlev] = (int)out.size();
  return out;
}
// the slabs of level `lev` whose box `rank` owns (owner[n][b]), as slab numbers, ascending
inline std::vector<int> diag_plan_local(const std::vector<DiagSlab> &slabs, int lev, const std::vector<int> *owner, int rank) {
  std::vector<int> out;
  for (int s = 0; s < (int)slabs.size(); s++)
    if (slabs[s].lev == lev && owner[lev][slabs[s].box] == rank) out.push_back(s);
  return out;
}
