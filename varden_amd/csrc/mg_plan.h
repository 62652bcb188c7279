// mg_plan.h -- the shape of a single-level multigrid hierarchy, decided once for the MAC and the nodal solver (cc_build in mg_cc.hip, nd_build in mg_nd.hip):
// which levels stay distributed box by box, which are gathered and replicated on every rank (the "tail"), where every box's data sits in the gather buffers
// and whether this rank holds the bottom level whole (the Krylov bottom solvers).  Plain host C++, integers only: no HIP, no ctx(), no sw() -- the testing
// program tests/cpp/mg_plan_check.cpp reads this header with a host compiler.  The builds keep what differs between the two multigrids: arrays, flags, plans.
#pragma once
#include <algorithm>
#include <array>
#include <cstdio>
#include <string>
#include <vector>

// the methods of the Krylov bottom solvers (krylov_wg.h) and the one mapping from mg_bottom_solver / hg_bottom_solver to them
#define VDN_KRYLOV_BICGSTAB 1
#define VDN_KRYLOV_CG 2
inline int mg_krylov_method(int bottom_solver) { return (bottom_solver == 1 || bottom_solver == 3) ? VDN_KRYLOV_BICGSTAB : (bottom_solver == 2 ? VDN_KRYLOV_CG : 0); }

// where a box's coarse cells sit in the first tail level (c0, n cells; nodes are n + 1) and in the all-gathered buffer (off): what the unpack kernels read
struct GBox { int c0[3]; int n[3]; long off; };
// one payload of the gather (cell-centred rhs, face coefficients, nodes, cells): rank r's buffer holds its boxes in local order, padded to maxloc boxes
struct MgGather {
  size_t cnt = 0;                 // doubles per rank
  std::vector<GBox> gb;           // per global box
  std::vector<long> loc_off;      // offsets of this rank's boxes inside its send buffer
};

struct MgDistLevel { int scale; int n[3]; /* box extent */ int ng[3]; /* global extents */ std::vector<std::array<int, 3>> lo; /* every global box's corner at this scale */ };
struct MgGatherBox { int c0[3]; int r, l; };      // coarse corner in the first tail level, owner, index among the owner's boxes
struct MgPlan {
  std::string err;                                // empty when all is well; else what is wrong with the box list (the levels planned so far stay)
  std::vector<MgDistLevel> dist;                  // distributed levels, finest first
  std::vector<std::array<int, 3>> tail;           // extents of the replicated levels; empty when the last distributed level is the bottom
  int rank = 0;
  int cn[3] = { 0, 0, 0 }; int maxloc = 0; std::vector<MgGatherBox> gbox;      // the gather into tail[0] (tail not empty): coarse box extent, most boxes on one rank
  bool whole_bottom = false; int bottom_n[3] = { 0, 0, 0 };                     // this rank holds the bottom level whole: the last tail level, or the last
                                                                                // distributed level of a hierarchy of more than one level made of one box
  bool second_dist_level() const { return dist.size() >= 2; }
  MgGather gather(long per) const {
    MgGather G; G.cnt = (size_t)per * maxloc;
    for (const MgGatherBox &b : gbox) {
      GBox g; for (int d = 0; d < 3; d++) { g.c0[d] = b.c0[d]; g.n[d] = cn[d]; }
      g.off = (long)b.r * (long)G.cnt + (long)b.l * per;
      G.gb.push_back(g);
      if (b.r == rank) G.loc_off.push_back((long)b.l * per);
    }
    return G;
  }
};

// Box: anything with lo[3], hi[3] (vdn_box).  agglom: mg_agglom(la, lev), the box width below which a multi-box level is gathered.
// The hierarchy of GLOBAL levels is the single-box one (oracle rule: coarsen while every global extent is even and > 2, at most 31 levels), and the arithmetic
// is that of the single-box hierarchy wherever the cut between distributed and gathered levels is made.
template <class Box>
MgPlan mg_plan(const Box *boxes, const int *owner, int nb, const Box &pd, int nranks, int rank, int agglom) {
  MgPlan P; P.rank = rank;
  // all boxes must share one size and be aligned to it (2x2x2-style decompositions); the general case needs per-box gather sizes
  int n[3]; for (int d = 0; d < 3; d++) n[d] = boxes[0].hi[d] - boxes[0].lo[d] + 1;
  for (int g = 0; g < nb; g++) for (int d = 0; d < 3; d++) {
    if (boxes[g].hi[d] - boxes[g].lo[d] + 1 != n[d]) { P.err = "all boxes of a level must have the same size"; return P; }
    if ((boxes[g].lo[d] - pd.lo[d]) % n[d] != 0) { P.err = "boxes must be aligned to their size"; return P; }
  }
  // several boxes: stop exchanging halos once the boxes get small -- every level that stays distributed costs ~10 latency-bound halo exchanges per V-cycle,
  // the replicated tail costs microseconds per pass; one box stays "distributed" while it halves cleanly to extents >= 4
  const int min_dist = nb > 1 ? agglom : 4;
  for (int scale = 1;; scale *= 2) {
    MgDistLevel L; L.scale = scale;
    for (int d = 0; d < 3; d++) { L.n[d] = n[d]; L.ng[d] = (pd.hi[d] - pd.lo[d] + 1) / scale; }
    for (int g = 0; g < nb; g++) L.lo.push_back({ (boxes[g].lo[0] - pd.lo[0]) / scale, (boxes[g].lo[1] - pd.lo[1]) / scale, (boxes[g].lo[2] - pd.lo[2]) / scale });
    P.dist.push_back(L);
    bool can = true, next_dist = true;
    for (int d = 0; d < 3; d++) { const int N = L.ng[d]; if ((N & 1) || N <= 2) can = false; }
    if (!can) break;                                   // the domain cannot be coarsened: this level is the bottom
    for (int d = 0; d < 3; d++) if (n[d] & 1) {
      char s[96]; snprintf(s, sizeof s, "box extent %d is odd while the domain can still be coarsened", n[d]);
      P.err = s; return P;
    }
    for (int d = 0; d < 3; d++) if (n[d] / 2 < min_dist || ((n[d] / 2) & 1)) next_dist = false;
    if (!next_dist) {                                  // the replicated tail starts at the half of this level
      std::array<int, 3> tn;
      for (int d = 0; d < 3; d++) { P.cn[d] = n[d] / 2; tn[d] = L.ng[d] / 2; }
      for (;;) {
        P.tail.push_back(tn);
        bool c2 = true;
        for (int d = 0; d < 3; d++) if ((tn[d] & 1) || tn[d] <= 2) c2 = false;
        if (!c2 || P.tail.size() >= 31) break;
        for (int d = 0; d < 3; d++) tn[d] /= 2;
      }
      std::vector<int> seen(nranks, 0);
      for (int g = 0; g < nb; g++) {
        MgGatherBox b; b.r = owner[g]; b.l = seen[b.r]++;
        for (int d = 0; d < 3; d++) b.c0[d] = L.lo[g][d] / 2;
        P.gbox.push_back(b);
        P.maxloc = std::max(P.maxloc, b.l + 1);
      }
      break;
    }
    for (int d = 0; d < 3; d++) n[d] /= 2;
    if (P.dist.size() >= 31) break;
  }
  if (!P.tail.empty()) { P.whole_bottom = true; for (int d = 0; d < 3; d++) P.bottom_n[d] = P.tail.back()[d]; }
  else if (P.dist.size() > 1 && nb == 1 && owner[0] == rank) { P.whole_bottom = true; for (int d = 0; d < 3; d++) P.bottom_n[d] = P.dist.back().n[d]; }
  return P;
}
