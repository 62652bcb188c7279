// diag_plan_check.cpp -- the slab split of vdn_diagnostics (varden_amd/csrc/diag_plan.h) held without a GPU: the slabs tile every box exactly once, come in
// (level, box, k) order, have the sizes the design states, and carry the same global numbers whichever rank owns a box.  Built with -fsanitize=address,undefined
// by tests/test_diagnostics_cpu.py.
#include "diag_plan.h"
#include <cstdio>
#include <cstdlib>

struct Box { int lo[3], hi[3]; };
static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { fails++; printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } } while (0)

static Box box(int a, int b, int c, int nx, int ny, int nz) { return Box{ { a, b, c }, { a + nx - 1, b + ny - 1, c + nz - 1 } }; }

// every plane of every box in exactly one slab, slabs ascending in (level, box, k), none larger than the bound unless it is one plane
static void check_tiling(int nlev, const std::vector<Box> *boxes) {
  int start[8];
  const std::vector<DiagSlab> s = diag_plan(nlev, boxes, start);
  CHECK(start[0] == 0 && start[nlev] == (int)s.size(), "level starts");
  size_t q = 0;
  for (int n = 0; n < nlev; n++) {
    CHECK(start[n] == (int)q, "level %d starts at %d, expected %zu", n, start[n], q);
    for (int b = 0; b < (int)boxes[n].size(); b++) {
      const Box &B = boxes[n][b];
      int next = B.lo[2];
      while (q < s.size() && s[q].lev == n && s[q].box == b) {
        CHECK(s[q].k0 == next && s[q].k1 >= s[q].k0 && s[q].k1 <= B.hi[2], "level %d box %d: slab %d..%d after plane %d", n, b, s[q].k0, s[q].k1, next);
        const long cells = (long)(B.hi[0] - B.lo[0] + 1) * (B.hi[1] - B.lo[1] + 1) * (s[q].k1 - s[q].k0 + 1);
        CHECK(cells <= DIAG_SLAB_CELLS || s[q].k1 == s[q].k0, "level %d box %d: a slab of %ld cells", n, b, cells);
        next = s[q].k1 + 1; q++;
      }
      CHECK(next == B.hi[2] + 1, "level %d box %d: planes up to %d covered, box ends at %d", n, b, next - 1, B.hi[2]);
    }
  }
  CHECK(q == s.size(), "%zu slabs in order, %zu in all", q, s.size());
}

int main() {
  int start[8];
  {   // the sizes DESIGN.md section 20 states
    std::vector<Box> one[1] = { { box(0, 0, 0, 48, 48, 40) } };
    std::vector<DiagSlab> s = diag_plan(1, one, start);
    CHECK(s.size() == 2 && s[0].k0 == 0 && s[0].k1 == 19 && s[1].k0 == 20 && s[1].k1 == 39, "48 x 48 x 40: two slabs of 20 planes expected, %zu slabs", s.size());
    std::vector<Box> small[1] = { { box(20, 12, 0, 20, 12, 28) } };
    s = diag_plan(1, small, start);
    CHECK(s.size() == 1 && s[0].k0 == 0 && s[0].k1 == 27, "20 x 12 x 28: one slab expected, %zu", s.size());
    std::vector<Box> flat[1] = { { box(0, 0, 0, 96, 64, 1), box(96, 0, 0, 32, 64, 1) } };      // dm = 2: one plane
    s = diag_plan(1, flat, start);
    CHECK(s.size() == 2 && s[0].k0 == 0 && s[0].k1 == 0 && s[1].box == 1 && s[1].k1 == 0, "dm = 2 boxes: one plane each");
    std::vector<Box> big[1] = { { box(0, 0, 0, 256, 256, 256), box(0, 0, 256, 512, 512, 3) } };   // a plane of 64 K cells, and one larger than the bound
    s = diag_plan(1, big, start);
    CHECK(s.size() == 259, "256^3: a slab per plane; 512 x 512 x 3: a slab per plane; %zu slabs", s.size());
    check_tiling(1, one); check_tiling(1, small); check_tiling(1, flat); check_tiling(1, big);
  }
  {   // a hierarchy: odd extents, lows away from zero, an empty level list entry is not a level
    std::vector<Box> h[3];
    for (int kz = 0; kz < 2; kz++) for (int ky = 0; ky < 2; ky++) for (int kx = 0; kx < 2; kx++) h[0].push_back(box(16 * kx, 16 * ky, 16 * kz, 16, 16, 16));
    h[1] = { box(8, 8, 8, 40, 44, 41), box(0, 0, 0, 8, 8, 8), box(48, 0, 0, 16, 64, 64) };
    h[2] = { box(32, 32, 32, 64, 64, 64), box(96, 32, 32, 17, 23, 129) };
    check_tiling(3, h);
    const std::vector<DiagSlab> s = diag_plan(3, h, start);
    // the global numbers do not depend on the owners: the local lists of any distribution partition 0 .. n-1, each ascending
    for (int nranks : { 1, 2, 3, 8 }) {
      std::vector<int> owner[3];
      for (int n = 0; n < 3; n++) for (size_t b = 0; b < h[n].size(); b++) owner[n].push_back((int)((b * 5 + n) % nranks));
      std::vector<int> seen(s.size(), 0);
      for (int r = 0; r < nranks; r++)
        for (int n = 0; n < 3; n++) {
          const std::vector<int> mine = diag_plan_local(s, n, owner, r);
          for (size_t i = 0; i < mine.size(); i++) {
            CHECK(mine[i] >= start[n] && mine[i] < start[n + 1], "rank %d level %d: slab %d outside the level", r, n, mine[i]);
            CHECK(i == 0 || mine[i] > mine[i - 1], "rank %d level %d: not ascending", r, n);
            CHECK(owner[n][s[mine[i]].box] == r, "rank %d was handed a foreign slab", r);
            seen[mine[i]]++;
          }
        }
      for (size_t i = 0; i < s.size(); i++) CHECK(seen[i] == 1, "%d ranks: slab %zu taken %d times", nranks, i, seen[i]);
    }
  }
  if (fails) { printf("%d checks failed\n", fails); return 1; }
  printf("OK\n");
  return 0;
}
