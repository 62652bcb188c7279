// particle_plan_check.cpp -- the box locator of the particle module (varden_amd/csrc/particle_plan.h) against a brute-force search, without a GPU: built with
// -fsanitize=address,undefined by tests/test_particles_cpu.py.  Every block of every level must name the one box that holds it (or -1 where no box does), every
// cell of the level must find its box through particle_map_index, the block size must be the largest that fits, and a level whose map would exceed the cap is
// refused with its number and block size in the message.
#include "particle_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

struct Box { int lo[3], hi[3]; };
static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); fails++; } } while (0)

static int brute(const std::vector<Box> &boxes, int i, int j, int k) {
  int found = -1;
  for (int b = 0; b < (int)boxes.size(); b++) {
    const Box &q = boxes[b];
    if (i >= q.lo[0] && i <= q.hi[0] && j >= q.lo[1] && j <= q.hi[1] && k >= q.lo[2] && k <= q.hi[2]) { if (found >= 0) return -2; found = b; }
  }
  return found;
}

static void check_level(const char *name, int lev, int n, const std::vector<Box> &boxes, const int want_blk[3]) {
  const Box pd = {{0, 0, 0}, {n - 1, n - 1, n - 1}};
  ParticleMap M;
  const std::string err = particle_plan(lev, boxes, pd, &M);
  CHECK(err.empty(), "%s level %d: refused: %s", name, lev, err.c_str());
  if (!err.empty()) return;
  for (int d = 0; d < 3; d++) {
    CHECK(M.blk[d] == want_blk[d], "%s level %d: block size %d along %d, expected %d", name, lev, M.blk[d], d, want_blk[d]);
    CHECK(M.n[d] * M.blk[d] == n, "%s level %d: %d blocks of %d do not tile %d cells", name, lev, M.n[d], M.blk[d], n);
  }
  CHECK((long)M.box.size() == (long)M.n[0] * M.n[1] * M.n[2], "%s level %d: map size", name, lev);
  // every block: all its cells agree with the brute-force search
  long wrong = 0;
  for (int k = 0; k < n; k++) for (int j = 0; j < n; j++) for (int i = 0; i < n; i++) {
    const int c[3] = {i, j, k};
    const long e = particle_map_index(c, M.lo, M.blk, M.n);
    if (e < 0 || e >= (long)M.box.size()) { wrong++; continue; }
    if (M.box[(size_t)e] != brute(boxes, i, j, k)) wrong++;
  }
  CHECK(wrong == 0, "%s level %d: %ld cells find another box than the search over all boxes", name, lev, wrong);
}

int main() {
  // amr2 and amr3 of tests/_diagnostics_worker.py
  {
    const std::vector<Box> l0 = {{{0, 0, 0}, {7, 15, 15}}, {{8, 0, 0}, {15, 15, 15}}};
    const std::vector<Box> l1 = {{{0, 8, 8}, {15, 23, 19}}, {{16, 8, 4}, {27, 19, 23}}};
    const int b0[3] = {8, 16, 16}, b1[3] = {4, 4, 4};
    check_level("amr2", 0, 16, l0, b0);
    check_level("amr2", 1, 32, l1, b1);
  }
  {
    std::vector<Box> l0;
    for (int k = 0; k < 2; k++) for (int j = 0; j < 2; j++) for (int i = 0; i < 2; i++) l0.push_back({{16 * i, 16 * j, 16 * k}, {16 * i + 15, 16 * j + 15, 16 * k + 15}});
    const std::vector<Box> l1 = {{{16, 16, 16}, {47, 47, 47}}, {{0, 16, 20}, {15, 31, 43}}};
    const std::vector<Box> l2 = {{{40, 40, 40}, {87, 75, 83}}};
    const int b0[3] = {16, 16, 16}, b1[3] = {16, 16, 4}, b2[3] = {8, 4, 4};
    check_level("amr3", 0, 32, l0, b0);
    check_level("amr3", 1, 64, l1, b1);
    check_level("amr3", 2, 128, l2, b2);
  }
  {   // an odd-aligned box: block size 1
    const std::vector<Box> l1 = {{{3, 5, 2}, {12, 9, 10}}};
    const int b[3] = {1, 1, 1};
    check_level("odd", 1, 32, l1, b);
  }
  {   // one box over the whole level: one block
    const std::vector<Box> l0 = {{{0, 0, 0}, {63, 63, 63}}};
    const int b[3] = {64, 64, 64};
    check_level("one", 0, 64, l0, b);
  }
  {   // no box at all: the whole domain is one empty block
    const std::vector<Box> none;
    const int b[3] = {8, 8, 8};
    check_level("empty", 2, 8, none, b);
  }
  {   // the cap: 512^3 blocks of one cell; nothing may be allocated for it
    const Box pd = {{0, 0, 0}, {511, 511, 511}};
    const std::vector<Box> l3 = {{{1, 1, 1}, {5, 5, 5}}};
    ParticleMap M;
    const std::string err = particle_plan(3, l3, pd, &M);
    CHECK(!err.empty(), "the cap: a 2^27-entry map was accepted");
    CHECK(err.find("level 3") != std::string::npos && err.find("1 x 1 x 1") != std::string::npos, "the cap: the message names neither level nor block size: %s", err.c_str());
    CHECK(M.box.empty(), "the cap: a refused map was filled");
    // just below: 2^25 entries exactly are legal
    const Box pd2 = {{0, 0, 0}, {511, 255, 255}};
    CHECK(particle_plan(3, l3, pd2, &M).empty() && (long)M.box.size() == PARTICLE_MAP_CAP, "the cap: 2^25 entries were refused");
  }
  {   // refusals of malformed lists
    const Box pd = {{0, 0, 0}, {15, 15, 15}};
    ParticleMap M;
    CHECK(!particle_plan(0, std::vector<Box>{{{0, 0, 0}, {16, 15, 15}}}, pd, &M).empty(), "a box outside the domain was accepted");
    CHECK(!particle_plan(0, std::vector<Box>{{{0, 0, 0}, {7, 15, 15}}, {{4, 0, 0}, {15, 15, 15}}}, pd, &M).empty(), "overlapping boxes were accepted");
  }
  if (fails) { printf("%d checks failed\n", fails); return 1; }
  printf("OK\n");
  return 0;
}
