// profile_plan_check.cpp -- the piece split and the bin tables of vdn_profiles (varden_amd/csrc/profile_plan.h) held without a GPU, for every axis: the pieces tile
// every box exactly once and keep the sizes the design states; the slots are numbered without gap in (level, box, piece) order; every cell index along the axis owns
// exactly the slots the level's table names, ascending; every fine bin reaches every box whose range contains m >> (L - l) through pieces that tile the box's
// cross-section exactly once; and nothing depends on who owns a box.  Built with -fsanitize=address,undefined by tests/test_profiles_cpu.py.
#include "profile_plan.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>

struct Box { int lo[3], hi[3]; };
static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static Box range(int x0, int x1, int y0, int y1, int z0, int z1) { return Box{ { x0, y0, z0 }, { x1, y1, z1 } }; }
static long cells(const int lo[3], const int hi[3]) { return (long)(hi[0] - lo[0] + 1) * (hi[1] - lo[1] + 1) * (hi[2] - lo[2] + 1); }

static void check_plan(const char *name, int nlev, const std::vector<Box> *boxes, const Box *dom, int axis) {
  const ProfPlan P = profile_plan(nlev, boxes, dom, axis);
  const int L = nlev - 1, c = prof_cut_dir(axis);
  CHECK(P.nbins == (long)(dom[0].hi[axis] - dom[0].lo[axis] + 1) << L, "%s axis %d: nbins %ld", name, axis, P.nbins);
  CHECK(P.piece_start[0] == 0 && P.slot_start[0] == 0 && P.piece_start[nlev] == (int)P.pieces.size(), "%s axis %d: starts", name, axis);
  // pieces: in (level, box) order, inside their box, slots back to back, sizes as designed; together they tile every box exactly once
  int slot = 0; size_t q = 0;
  for (int l = 0; l < nlev; l++) {
    CHECK(P.piece_start[l] == (int)q && P.slot_start[l] == slot, "%s axis %d: level %d starts at piece %d slot %d, expected %zu %d", name, axis, l, P.piece_start[l], P.slot_start[l], q, slot);
    CHECK(P.na[l] == (dom[0].hi[axis] - dom[0].lo[axis] + 1) << l, "%s axis %d: level %d has %d cells along the axis", name, axis, l, P.na[l]);
    for (int b = 0; b < (int)boxes[l].size(); b++) {
      const Box &B = boxes[l][b];
      const int n[3] = { B.hi[0] - B.lo[0] + 1, B.hi[1] - B.lo[1] + 1, B.hi[2] - B.lo[2] + 1 };
      std::vector<unsigned char> seen((size_t)cells(B.lo, B.hi), 0);
      while (q < P.pieces.size() && P.pieces[q].lev == l && P.pieces[q].box == b) {
        const ProfPiece &p = P.pieces[q];
        CHECK(p.slot0 == slot, "%s axis %d: piece %zu starts at slot %d, expected %d", name, axis, q, p.slot0, slot);
        bool inside = true;
        for (int d = 0; d < 3; d++) inside = inside && p.lo[d] >= B.lo[d] && p.hi[d] <= B.hi[d] && p.lo[d] <= p.hi[d];
        CHECK(inside, "%s axis %d: piece %zu leaves its box", name, axis, q);
        if (!inside) { q++; continue; }
        if (axis == 0) {
          CHECK(p.hi[0] - p.lo[0] + 1 <= PROF_XW, "%s: a piece %d cells wide along x", name, p.hi[0] - p.lo[0] + 1);
          CHECK(p.lo[1] == B.lo[1] && p.hi[1] == B.hi[1], "%s axis 0: a piece is cut along y", name);
          CHECK((long)PROF_XW * n[1] * (p.hi[2] - p.lo[2] + 1) <= PROF_PIECE_CELLS || p.hi[2] == p.lo[2], "%s axis 0: a piece of %d planes", name, p.hi[2] - p.lo[2] + 1);
        } else {
          CHECK(p.lo[0] == B.lo[0] && p.hi[0] == B.hi[0] && p.lo[axis] == B.lo[axis] && p.hi[axis] == B.hi[axis], "%s axis %d: a piece is cut along x or the axis", name, axis);
          CHECK((long)n[0] * (p.hi[c] - p.lo[c] + 1) <= PROF_PIECE_CELLS || p.hi[c] == p.lo[c], "%s axis %d: a cross-section of %ld cells", name, axis, (long)n[0] * (p.hi[c] - p.lo[c] + 1));
        }
        for (int k = p.lo[2]; k <= p.hi[2]; k++) for (int j = p.lo[1]; j <= p.hi[1]; j++) for (int i = p.lo[0]; i <= p.hi[0]; i++)
          seen[((size_t)(k - B.lo[2]) * n[1] + (j - B.lo[1])) * n[0] + (i - B.lo[0])]++;
        slot += p.hi[axis] - p.lo[axis] + 1; q++;
      }
      size_t bad = 0;
      for (unsigned char s : seen) bad += s != 1;
      CHECK(bad == 0, "%s axis %d: level %d box %d: %zu cells not in exactly one piece", name, axis, l, b, bad);
    }
  }
  CHECK(q == P.pieces.size() && slot == P.slot_start[nlev], "%s axis %d: %zu pieces in order of %zu, %d slots of %d", name, axis, q, P.pieces.size(), slot, P.slot_start[nlev]);
  // tables: row i of level l names exactly the slots of the level's pieces that span i, ascending
  std::vector<int> used(slot, 0);
  for (int l = 0; l < nlev; l++) {
    CHECK((int)P.ptr[l].size() == P.na[l] + 1 && P.ptr[l][0] == 0 && P.ptr[l][P.na[l]] == (int)P.idx[l].size(), "%s axis %d: level %d: the table's frame", name, axis, l);
    for (int i = 0; i < P.na[l]; i++) {
      std::vector<int> want;
      for (int p = P.piece_start[l]; p < P.piece_start[l + 1]; p++)
        if (P.pieces[p].lo[axis] <= i + dom[l].lo[axis] && i + dom[l].lo[axis] <= P.pieces[p].hi[axis]) want.push_back(P.pieces[p].slot0 + i + dom[l].lo[axis] - P.pieces[p].lo[axis]);
      const std::vector<int> got(P.idx[l].begin() + P.ptr[l][i], P.idx[l].begin() + P.ptr[l][i + 1]);
      CHECK(got == want, "%s axis %d: level %d row %d: %zu slots named, %zu owned", name, axis, l, i, got.size(), want.size());
      for (size_t s = 0; s + 1 < got.size(); s++) CHECK(got[s] < got[s + 1], "%s axis %d: level %d row %d: slots not ascending", name, axis, l, i);
      for (int s : got) if (s >= 0 && s < slot) used[s]++;
    }
  }
  for (int s = 0; s < slot; s++) CHECK(used[s] == 1, "%s axis %d: slot %d is named %d times", name, axis, s, used[s]);
  // bins: bin m reaches, on every level, every box whose range contains m >> (L - l), through pieces whose cross-sections add up to the box's -- exactly once
  for (long m = 0; m < P.nbins; m++)
    for (int l = 0; l < nlev; l++) {
      const int ci = (int)(m >> (L - l));
      std::vector<long> area(boxes[l].size(), 0);
      for (int s = P.ptr[l][ci]; s < P.ptr[l][ci + 1]; s++) {
        int p = P.piece_start[l];
        while (p + 1 < P.piece_start[l + 1] && P.pieces[p + 1].slot0 <= P.idx[l][s]) p++;
        const ProfPiece &pc = P.pieces[p];
        area[pc.box] += cells(pc.lo, pc.hi) / (pc.hi[axis] - pc.lo[axis] + 1);
      }
      for (int b = 0; b < (int)boxes[l].size(); b++) {
        const Box &B = boxes[l][b];
        const bool in = B.lo[axis] <= ci + dom[l].lo[axis] && ci + dom[l].lo[axis] <= B.hi[axis];
        const long want = in ? cells(B.lo, B.hi) / (B.hi[axis] - B.lo[axis] + 1) : 0;
        CHECK(area[b] == want, "%s axis %d: bin %ld level %d box %d: %ld cells reached, %ld in the cross-section", name, axis, m, l, b, area[b], want);
      }
    }
  // owners: the plan never sees them; the local lists of any distribution partition the pieces, each ascending
  const ProfPlan again = profile_plan(nlev, boxes, dom, axis);
  for (int l = 0; l < nlev; l++) CHECK(again.ptr[l] == P.ptr[l] && again.idx[l] == P.idx[l], "%s axis %d: level %d: two plans differ", name, axis, l);
  for (int nranks : { 1, 2, 3, 8 }) {
    std::vector<int> owner[PROF_MAXLEV];
    for (int l = 0; l < nlev; l++) for (size_t b = 0; b < boxes[l].size(); b++) owner[l].push_back((int)((b * 5 + l) % nranks));
    std::vector<int> taken(P.pieces.size(), 0);
    for (int r = 0; r < nranks; r++)
      for (int l = 0; l < nlev; l++) {
        const std::vector<int> mine = profile_plan_local(P, l, owner, r);
        for (size_t i = 0; i < mine.size(); i++) {
          CHECK(mine[i] >= P.piece_start[l] && mine[i] < P.piece_start[l + 1] && (i == 0 || mine[i] > mine[i - 1]), "%s: rank %d level %d: piece %d out of order", name, r, l, mine[i]);
          CHECK(owner[l][P.pieces[mine[i]].box] == r, "%s: rank %d was handed a foreign piece", name, r);
          taken[mine[i]]++;
        }
      }
    for (size_t i = 0; i < taken.size(); i++) CHECK(taken[i] == 1, "%s: %d ranks: piece %zu taken %d times", name, nranks, i, taken[i]);
  }
}

int main() {
  {   // one level: one box whose extents are no multiple of the wave width; 32 x 16 x 24 cut into 2 x 1 x 3 boxes
    const Box dom[1] = { range(0, 11, 0, 19, 0, 7) };
    std::vector<Box> one[1] = { { dom[0] } };
    for (int a = 0; a < 3; a++) check_plan("12x20x8", 1, one, dom, a);
    const Box dom2[1] = { range(0, 31, 0, 15, 0, 23) };
    std::vector<Box> six[1];
    for (int k = 0; k < 3; k++) for (int i = 0; i < 2; i++) six[0].push_back(range(16 * i, 16 * i + 15, 0, 15, 8 * k, 8 * k + 7));
    for (int a = 0; a < 3; a++) check_plan("32x16x24", 1, six, dom2, a);
  }
  {   // three levels: a 16^3 base in two boxes, two level-1 boxes that are not aligned and abut nowhere, one level-2 box inside the first
    const Box dom[3] = { range(0, 15, 0, 15, 0, 15), range(0, 31, 0, 31, 0, 31), range(0, 63, 0, 63, 0, 63) };
    std::vector<Box> h[3];
    h[0] = { range(0, 7, 0, 15, 0, 15), range(8, 15, 0, 15, 0, 15) };
    h[1] = { range(8, 19, 8, 23, 4, 15), range(20, 27, 8, 15, 16, 31) };
    h[2] = { range(20, 35, 20, 43, 12, 27) };
    for (int a = 0; a < 3; a++) check_plan("amr3", 3, h, dom, a);
    for (int a = 0; a < 3; a++) check_plan("amr3, two levels", 2, h, dom, a);
  }
  {   // dm = 2: 24 x 40 in two boxes, one plane along z; a degenerate one-cell box; a domain whose low corner is not zero
    const Box dom[1] = { range(0, 23, 0, 39, 0, 0) };
    std::vector<Box> two[1] = { { range(0, 23, 0, 19, 0, 0), range(0, 23, 20, 39, 0, 0) } };
    for (int a = 0; a < 2; a++) check_plan("24x40", 1, two, dom, a);
    const Box cell[1] = { range(0, 0, 0, 0, 0, 0) };
    std::vector<Box> c1[1] = { { cell[0] } };
    for (int a = 0; a < 3; a++) check_plan("one cell", 1, c1, cell, a);
    const Box off[2] = { range(4, 11, -2, 5, 8, 15), range(8, 23, -4, 11, 16, 31) };
    std::vector<Box> ho[2] = { { off[0] }, { range(10, 17, -2, 5, 20, 27) } };
    for (int a = 0; a < 3; a++) check_plan("offset domain", 2, ho, off, a);
  }
  {   // the sizes DESIGN.md section 22 states
    const Box dom[1] = { range(0, 255, 0, 255, 0, 255) };
    std::vector<Box> big[1] = { { dom[0] } };
    ProfPlan P = profile_plan(1, big, dom, 0);
    CHECK(P.pieces.size() == 256 && P.slot_start[1] == 256 * 64 && P.pieces[0].hi[2] == 3, "256^3 along x: 4 x 64 pieces of 64 slots and 4 planes expected, %zu pieces", P.pieces.size());
    P = profile_plan(1, big, dom, 1);
    CHECK(P.pieces.size() == 1 && P.slot_start[1] == 256, "256^3 along y: one piece of 256 slots expected, %zu pieces", P.pieces.size());
    P = profile_plan(1, big, dom, 2);
    CHECK(P.pieces.size() == 1 && P.slot_start[1] == 256, "256^3 along z: one piece of 256 slots expected, %zu pieces", P.pieces.size());
    const Box wd[1] = { range(0, 511, 0, 511, 0, 3) };
    std::vector<Box> wide[1] = { { wd[0] } };
    P = profile_plan(1, wide, wd, 2);
    CHECK(P.pieces.size() == 4 && P.slot_start[1] == 16 && P.ptr[0][1] == 4, "512 x 512 x 4 along z: four pieces of 128 rows, four slots per bin; %zu pieces", P.pieces.size());
    for (int a = 0; a < 3; a++) check_plan("512x512x4", 1, wide, wd, a);
  }
  if (fails) { printf("%d checks failed\n", fails); return 1; }
  printf("OK\n");
  return 0;
}
