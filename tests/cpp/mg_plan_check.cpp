// The hierarchy rule of varden_amd/csrc/mg_plan.h, without a GPU and without the library: the shapes cc_build and nd_build derived before the rule had one
// home (worked out by hand from cc_build), the level count of the oracle's rule (oracle/vo_macproject.c: coarsen while every global extent is even and > 2,
// at most 31 levels -- written here again as its own loop), the gather offsets, the three input errors and the bottom-solver mapping.
// Built and run by tests/test_mg_plan_cpu.py.
#include "mg_plan.h"
#include <cstdio>
#include <string>
#include <vector>

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_bad++; fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

struct Box { int lo[3], hi[3]; };
typedef std::array<int, 3> I3;

// a domain of N cells from `origin` on, cut into boxes of bn cells, x fastest
static std::vector<Box> cut(const I3 &N, const I3 &bn, int origin = 0) {
  std::vector<Box> v;
  for (int k = 0; k < N[2] / bn[2]; k++) for (int j = 0; j < N[1] / bn[1]; j++) for (int i = 0; i < N[0] / bn[0]; i++) {
    const int q[3] = { i, j, k };
    Box b; for (int d = 0; d < 3; d++) { b.lo[d] = origin + q[d] * bn[d]; b.hi[d] = b.lo[d] + bn[d] - 1; }
    v.push_back(b);
  }
  return v;
}
static Box domain(const I3 &N, int origin = 0) { Box b; for (int d = 0; d < 3; d++) { b.lo[d] = origin; b.hi[d] = origin + N[d] - 1; } return b; }
static int oracle_levels(I3 n) {
  int nlev = 1;
  while (nlev < 31 && !((n[0] & 1) || n[0] <= 2 || (n[1] & 1) || n[1] <= 2 || (n[2] & 1) || n[2] <= 2)) { for (int d = 0; d < 3; d++) n[d] /= 2; nlev++; }
  return nlev;
}
static MgPlan plan(const I3 &N, const I3 &bn, int agglom, std::vector<int> owner = {}, int nranks = 1, int rank = 0, int origin = 0) {
  const std::vector<Box> b = cut(N, bn, origin);
  owner.resize(b.size(), 0);
  return mg_plan(b.data(), owner.data(), (int)b.size(), domain(N, origin), nranks, rank, agglom);
}
// the plan against: box extents of the distributed levels, global extents of the tail levels
static void shape(const char *what, const I3 &N, const MgPlan &P, const std::vector<I3> &dist, const std::vector<I3> &tail) {
  CHECK(P.err.empty(), "%s: %s", what, P.err.c_str());
  CHECK(P.dist.size() == dist.size() && P.tail.size() == tail.size(), "%s: %zu + %zu levels", what, P.dist.size(), P.tail.size());
  CHECK((int)(P.dist.size() + P.tail.size()) == oracle_levels(N), "%s: %zu levels, the oracle's rule gives %d", what, P.dist.size() + P.tail.size(), oracle_levels(N));
  if (P.dist.size() != dist.size() || P.tail.size() != tail.size()) return;
  for (size_t l = 0; l < dist.size(); l++) for (int d = 0; d < 3; d++) {
    CHECK(P.dist[l].n[d] == dist[l][d] && P.dist[l].scale == 1 << l && P.dist[l].ng[d] == N[d] >> l, "%s: level %zu: n %d scale %d ng %d", what, l, P.dist[l].n[d], P.dist[l].scale, P.dist[l].ng[d]);
  }
  for (size_t l = 0; l < tail.size(); l++) CHECK(P.tail[l] == tail[l], "%s: tail level %zu: %d %d %d", what, l, P.tail[l][0], P.tail[l][1], P.tail[l][2]);
  const bool whole = !tail.empty() || dist.size() > 1;      // (every case here is one rank's: several boxes always end in a tail)
  const I3 bottom = !tail.empty() ? tail.back() : dist.back();
  CHECK(P.whole_bottom == whole, "%s: whole bottom %d", what, (int)P.whole_bottom);
  if (whole) CHECK(P.bottom_n[0] == bottom[0] && P.bottom_n[1] == bottom[1] && P.bottom_n[2] == bottom[2], "%s: bottom %d %d %d", what, P.bottom_n[0], P.bottom_n[1], P.bottom_n[2]);
}
static I3 cube(int n) { return I3{ n, n, n }; }
static std::vector<I3> cubes(std::initializer_list<int> l) { std::vector<I3> v; for (int n : l) v.push_back(cube(n)); return v; }

int main() {
  // ---- shapes ----
  const MgPlan r1 = plan(cube(256), cube(256), 64);
  shape("256^3, one box", cube(256), r1, cubes({ 256, 128, 64, 32, 16, 8, 4 }), cubes({ 2 }));
  shape("200^3, one box", cube(200), plan(cube(200), cube(200), 64), cubes({ 200, 100, 50 }), cubes({ 25 }));
  shape("132 x 36 x 40, one box", I3{ 132, 36, 40 }, plan(I3{ 132, 36, 40 }, I3{ 132, 36, 40 }, 64), { I3{ 132, 36, 40 }, I3{ 66, 18, 20 } }, { I3{ 33, 9, 10 } });
  const MgPlan r4 = plan(cube(25), cube(25), 64);
  shape("25^3, one box", cube(25), r4, cubes({ 25 }), {});
  CHECK(!r4.whole_bottom, "a one-level hierarchy has no whole bottom");
  const MgPlan r5 = plan(cube(256), cube(128), 64);
  shape("256^3 in eight boxes, agglom 64", cube(256), r5, cubes({ 128, 64 }), cubes({ 64, 32, 16, 8, 4, 2 }));
  CHECK(r5.cn[0] == 32 && r5.cn[1] == 32 && r5.cn[2] == 32, "cn %d", r5.cn[0]);
  const MgPlan r6 = plan(cube(256), cube(128), 128);
  shape("256^3 in eight boxes, agglom 128", cube(256), r6, cubes({ 128 }), cubes({ 128, 64, 32, 16, 8, 4, 2 }));
  CHECK(r6.cn[0] == 64 && r6.cn[1] == 64 && r6.cn[2] == 64, "cn %d", r6.cn[0]);
  // the tail is every rank's, whoever owns the boxes above it
  CHECK(plan(cube(64), cube(64), 64, { 1 }, 2, 0).whole_bottom && plan(cube(64), cube(64), 64, { 1 }, 2, 1).whole_bottom, "a tail's bottom is whole on every rank");
  // corners: at every scale, relative to the domain's first cell
  {
    const MgPlan p = plan(cube(256), cube(128), 64, {}, 1, 0, /* origin */ 128);
    shape("256^3 in eight boxes from 128 on", cube(256), p, cubes({ 128, 64 }), cubes({ 64, 32, 16, 8, 4, 2 }));
    CHECK(p.dist[0].lo[7] == cube(128) && p.dist[1].lo[7] == cube(64) && p.dist[1].lo[2] == (I3{ 0, 64, 0 }), "corners %d %d", p.dist[0].lo[7][0], p.dist[1].lo[7][0]);
    CHECK(p.gbox[7].c0[0] == 32 && p.gbox[2].c0[0] == 0 && p.gbox[2].c0[1] == 32 && p.gbox[2].c0[2] == 0, "coarse corners");
  }
  // ---- a second distributed level ----
  CHECK(r1.second_dist_level() && r5.second_dist_level(), "rows 1 and 5 have a second distributed level");
  CHECK(!r4.second_dist_level() && !r6.second_dist_level(), "rows 4 and 6 have none");
  CHECK(!plan(cube(128), cube(64), 64).second_dist_level(), "eight 64^3 boxes, agglom 64: none");
  // ---- gather ----
  {
    const std::vector<int> owner = { 0, 1, 2, 0, 1, 2, 0, 1 };
    const MgPlan p = plan(cube(256), cube(128), 64, owner, 3, 2);
    const long per = (long)p.cn[0] * p.cn[1] * p.cn[2];
    const MgGather G = p.gather(per);
    CHECK(p.maxloc == 3 && p.gbox.size() == 8 && G.gb.size() == 8, "maxloc %d", p.maxloc);
    CHECK(p.gbox[6].r == 0 && p.gbox[6].l == 2 && p.gbox[7].r == 1 && p.gbox[7].l == 2, "boxes 6, 7: (%d, %d), (%d, %d)", p.gbox[6].r, p.gbox[6].l, p.gbox[7].r, p.gbox[7].l);
    CHECK(per == 32L * 32 * 32 && G.cnt == (size_t)(3 * per) && G.gb[7].off == 1 * 3 * per + 2 * per, "cnt %zu off %ld", G.cnt, G.gb[7].off);
    CHECK(G.gb[7].n[0] == 32 && G.gb[7].c0[0] == 32 && G.gb[7].c0[1] == 32 && G.gb[7].c0[2] == 32, "box 7 in the tail level");
    CHECK(G.loc_off.size() == 2 && G.loc_off[0] == 0 && G.loc_off[1] == per, "rank 2's local offsets");
    const long pern = 33L * 33 * 33;
    CHECK(p.gather(pern).gb[5].off == 2 * 3 * pern + 1 * pern && p.gather(pern).loc_off[1] == pern, "the same with another payload");
  }
  // ---- errors ----
  {
    std::vector<Box> b = cut(I3{ 64, 32, 32 }, cube(32));
    const std::vector<int> owner(2, 0);
    b[1].hi[0] -= 16;
    CHECK(mg_plan(b.data(), owner.data(), 2, domain(I3{ 64, 32, 32 }), 1, 0, 64).err == "all boxes of a level must have the same size", "two sizes");
    b = cut(I3{ 64, 32, 32 }, cube(32));
    b[1].lo[0] += 8; b[1].hi[0] += 8;
    const MgPlan p = mg_plan(b.data(), owner.data(), 2, domain(I3{ 72, 32, 32 }), 1, 0, 64);
    CHECK(p.err == "boxes must be aligned to their size", "misaligned: %s", p.err.c_str());
    CHECK(!p.second_dist_level() && !p.whole_bottom, "a plan with an error promises nothing");
    CHECK(plan(cube(20), cube(5), 64).err == "box extent 5 is odd while the domain can still be coarsened", "odd boxes: %s", plan(cube(20), cube(5), 64).err.c_str());
  }
  // ---- method mapping ----
  const int want[6] = { 0, 0, VDN_KRYLOV_BICGSTAB, VDN_KRYLOV_CG, VDN_KRYLOV_BICGSTAB, 0 };
  for (int b = -1; b <= 4; b++) CHECK(mg_krylov_method(b) == want[b + 1], "bottom solver %d: method %d", b, mg_krylov_method(b));
  CHECK(VDN_KRYLOV_BICGSTAB != 0 && VDN_KRYLOV_CG != 0 && VDN_KRYLOV_BICGSTAB != VDN_KRYLOV_CG, "methods");
  if (g_bad) { printf("%d checks failed\n", g_bad); return 1; }
  printf("OK\n");
  return 0;
}
