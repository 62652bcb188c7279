// profile_plan.h -- the piece split and the bin tables of vdn_profiles (profiles.hip), host only: no HIP, no library type, so tests/cpp/profile_plan_check.cpp holds
// it without a GPU.
//
// Bins are the planes of the FINEST level's index space along the axis a.  Every box is cut into PIECES; a piece is a sub-box and owns one SLOT of partials per cell
// index along a that it spans (hi[a] - lo[a] + 1 of them, slot0 first).  Pieces and slots are numbered in (level, global box, piece) order from the GLOBAL box lists
// alone: the number of a slot does not depend on which rank owns its box, and the final sum of a bin runs over the slots in that order on every rank.
//   a = 0   a piece is at most PROF_XW cells wide along x (a lane of a wave owns an i) and a run of whole k-planes of about PROF_PIECE_CELLS cells
//   a = 1   a piece spans the box along y and x and a run of whole k-planes: one (x, z) cross-section of it holds at most PROF_PIECE_CELLS cells (or one row)
//   a = 2   a piece spans the box along z and x and a run of whole j-rows: one (x, y) cross-section of it holds at most PROF_PIECE_CELLS cells (or one row)
// Per level the table "cell index along a (counted from the level's domain) -> the slots to add, ascending" is kept in CSR form (ptr, idx).  Bin m of a hierarchy
// whose finest level is L adds, for l = 0 .. L, the slots of row (m >> (L - l)) of level l's table.
#pragma once
#include <vector>

constexpr long PROF_PIECE_CELLS = 65536;
constexpr int PROF_XW = 64;
constexpr int PROF_MAXLEV = 4;

struct ProfPiece { int lev, box; int lo[3], hi[3]; int slot0; };      // box: the global index on its level
struct ProfPlan {
  int axis = 0, nlev = 0;
  long nbins = 0;
  int na[PROF_MAXLEV] = {0, 0, 0, 0};                 // cells of level l's domain along the axis
  int piece_start[PROF_MAXLEV + 1] = {0, 0, 0, 0, 0}; // level l's pieces: piece_start[l] .. piece_start[l + 1] - 1
  int slot_start[PROF_MAXLEV + 1] = {0, 0, 0, 0, 0};  // ... and its slots; slot_start[nlev]: their count
  std::vector<ProfPiece> pieces;
  std::vector<int> ptr[PROF_MAXLEV], idx[PROF_MAXLEV]; // ptr[l]: na[l] + 1 entries
};

// the direction a box is cut along besides the axis (and, for a = 0, besides x)
inline int prof_cut_dir(int axis) { return axis == 2 ? 1 : 2; }
// whole rows / planes along the cut direction per piece: `per` cells of the cross-section lie in one of them; spread evenly over the pieces
inline int prof_cut_len(long per, int n) {
  long q = PROF_PIECE_CELLS / (per > 0 ? per : 1);
  if (q < 1) q = 1;
  if (q > n) q = n;
  const int np = (int)((n + q - 1) / q);
  return (n + np - 1) / np;
}

// B: anything with int lo[3], hi[3].  boxes[l]: the global box list of level l; dom[l]: the level's domain.  Empty boxes own nothing.
template <class B>
inline ProfPlan profile_plan(int nlev, const std::vector<B> *boxes, const B *dom, int axis) {
  ProfPlan P;
  P.axis = axis; P.nlev = nlev;
  const int c = prof_cut_dir(axis);
  int slot = 0;
  for (int l = 0; l < nlev; l++) {
    P.na[l] = dom[l].hi[axis] - dom[l].lo[axis] + 1;
    P.piece_start[l] = (int)P.pieces.size(); P.slot_start[l] = slot;
    for (int b = 0; b < (int)boxes[l].size(); b++) {
      const B &q = boxes[l][b];
      if (q.hi[0] < q.lo[0] || q.hi[1] < q.lo[1] || q.hi[2] < q.lo[2]) continue;
      const int nx = q.hi[0] - q.lo[0] + 1, ny = q.hi[1] - q.lo[1] + 1, nc = q.hi[c] - q.lo[c] + 1;
      // cells of one unit along the cut direction: a = 0: a plane's rows (a lane per i: PROF_XW cells each, whatever the piece's width); otherwise one x row
      const int len = prof_cut_len(axis == 0 ? (long)PROF_XW * ny : (long)nx, nc);
      const int xw = axis == 0 ? PROF_XW : nx;
      for (int c0 = q.lo[c]; c0 <= q.hi[c]; c0 += len)
        for (int i0 = q.lo[0]; i0 <= q.hi[0]; i0 += xw) {
          ProfPiece p; p.lev = l; p.box = b; p.slot0 = slot;
          for (int d = 0; d < 3; d++) { p.lo[d] = q.lo[d]; p.hi[d] = q.hi[d]; }
          p.lo[c] = c0; p.hi[c] = c0 + len - 1 < q.hi[c] ? c0 + len - 1 : q.hi[c];
          p.lo[0] = i0; p.hi[0] = i0 + xw - 1 < q.hi[0] ? i0 + xw - 1 : q.hi[0];
          slot += p.hi[axis] - p.lo[axis] + 1;
          P.pieces.push_back(p);
        }
    }
    // the level's table: count, prefix, fill -- pieces in ascending order, so every row's slots ascend
    const int na = P.na[l], d0 = dom[l].lo[axis];
    P.ptr[l].assign(na + 1, 0);
    for (int p = P.piece_start[l]; p < (int)P.pieces.size(); p++)
      for (int i = P.pieces[p].lo[axis]; i <= P.pieces[p].hi[axis]; i++)
        if (i - d0 >= 0 && i - d0 < na) P.ptr[l][i - d0 + 1]++;
    for (int i = 0; i < na; i++) P.ptr[l][i + 1] += P.ptr[l][i];
    P.idx[l].assign(P.ptr[l][na], 0);
    std::vector<int> fill(P.ptr[l].begin(), P.ptr[l].end() - 1);
    for (int p = P.piece_start[l]; p < (int)P.pieces.size(); p++)
      for (int i = P.pieces[p].lo[axis]; i <= P.pieces[p].hi[axis]; i++)
        if (i - d0 >= 0 && i - d0 < na) P.idx[l][fill[i - d0]++] = P.pieces[p].slot0 + (i - P.pieces[p].lo[axis]);
  }
  P.piece_start[nlev] = (int)P.pieces.size(); P.slot_start[nlev] = slot;
  P.nbins = nlev > 0 ? (long)P.na[0] << (nlev - 1) : 0;
  return P;
}

// the pieces of level `lev` whose box `rank` owns (owner[l][b]), as piece numbers, ascending
inline std::vector<int> profile_plan_local(const ProfPlan &P, int lev, const std::vector<int> *owner, int rank) {
  std::vector<int> out;
  for (int p = P.piece_start[lev]; p < P.piece_start[lev + 1]; p++)
    if (owner[lev][P.pieces[p].box] == rank) out.push_back(p);
  return out;
}
