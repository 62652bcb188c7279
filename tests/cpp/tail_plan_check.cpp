// The arithmetic of varden_amd/csrc/tail_plan.h, without a GPU and without the library.  For every level set that the multigrid builds can hand a tail cycle
// for one box of up to 64^3 cells (the single-box hierarchy: halve while every extent is even and > 2; the tail is the levels of at most 512 cells, two at
// least), cells and nodes, with no periodic axis, one, and all three: `fits` is true exactly when the rules and the LDS budget, worked out here once more, allow
// it; then every cell or node of every level is owned by exactly one of the 1024 threads, a cell's colour is (i + j + k) & 1 and the threads of colour 0 come
// first, the index of a ghosted array is one-to-one onto it, and the arrays in LDS neither overlap nor pass the budget.  The extreme shapes that the point
// bounds admit (1 x 1 x 512, 2 x 2 x 128, 8 x 4 x 16 cells; 9^3, 5 x 3 x 33 nodes) the same way, and level sets that must be refused.
// Built and run by tests/test_tail_plan_cpu.py, also with -fsanitize=address,undefined.
#include "tail_plan.h"
#include <algorithm>
#include <array>
#include <cstdio>
#include <utility>
#include <vector>

static int g_bad = 0;
static long g_sets = 0, g_fit = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_bad++ < 20) { fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } } while (0)

// every point of a level is owned once
static void check_owners(int kind, const int n[3]) {
  const int m[3] = { n[0] + kind, n[1] + kind, n[2] + kind };
  std::vector<int> seen((size_t)m[0] * m[1] * m[2], 0);
  int last_colour = 0;
  CHECK(tail_threads(kind, n) <= TAIL_THREADS, "kind %d %d x %d x %d: threads", kind, n[0], n[1], n[2]);
  for (int t = -1; t <= TAIL_THREADS; t++) {
    int i, j, k, c;
    if (!tail_owner(kind, n, t, i, j, k, c)) continue;
    CHECK(t >= 0 && t < TAIL_THREADS, "thread %d owns a point", t);
    const bool in = i >= 0 && i < m[0] && j >= 0 && j < m[1] && k >= 0 && k < m[2];
    CHECK(in, "kind %d %d x %d x %d thread %d: (%d, %d, %d)", kind, n[0], n[1], n[2], t, i, j, k);
    if (!in) continue;
    seen[(size_t)i + (size_t)m[0] * (j + (size_t)m[1] * k)]++;
    if (kind == TAIL_CELLS) {
      CHECK(c == ((i + j + k) & 1), "thread %d: colour %d of cell (%d, %d, %d)", t, c, i, j, k);
      CHECK(c >= last_colour, "thread %d: colour 0 after colour 1", t);
      last_colour = c;
    }
  }
  for (size_t q = 0; q < seen.size(); q++) CHECK(seen[q] == 1, "kind %d %d x %d x %d: point %zu owned %d times", kind, n[0], n[1], n[2], q, seen[q]);
}

// what tail_plan must answer, from the rules written in tail_plan.h
static bool expect_fits(int kind, int nlev, const int (*n)[3], const int per[3], long &total) {
  total = 0;
  if (nlev < 2 || nlev > TAIL_MAX_LEVELS) return false;
  bool ok = true;
  for (int l = 0; l < nlev; l++) {
    long pts = 1, cells = 1, arr = 1, sig = 1;
    for (int d = 0; d < 3; d++) {
      if (n[l][d] < 1) return false;
      cells *= n[l][d]; pts *= n[l][d] + kind; arr *= n[l][d] + 2 + kind; sig *= n[l][d] + 2;
      if (l > 0 && 2 * n[l][d] != n[l - 1][d]) ok = false;
      if (per[d] && (kind == TAIL_NODES || n[l][d] % 2)) ok = false;
    }
    const long threads = kind == TAIL_CELLS ? 2L * ((n[l][0] + 1) / 2) * n[l][1] * n[l][2] : pts;
    if (threads > TAIL_THREADS || cells > TAIL_THREADS) return false;
    total += kind == TAIL_CELLS ? arr : 3 * arr + sig;
  }
  if (kind == TAIL_CELLS) total += (long)n[0][0] * n[0][1] * n[0][2];
  return ok && total <= TAIL_LDS_DOUBLES;
}

static void check_set(int kind, int nlev, const int (*n)[3], const int per[3]) {
  g_sets++;
  const TailPlan P = tail_plan(kind, nlev, n, per);
  long total;
  const bool want = expect_fits(kind, nlev, n, per, total);
  CHECK((P.fits != 0) == want, "kind %d, %d levels from %d x %d x %d, per %d%d%d: fits %d, expected %d", kind, nlev, n[0][0], n[0][1], n[0][2], per[0], per[1], per[2], P.fits, (int)want);
  if (!P.fits) return;
  g_fit++;
  CHECK(P.total == total && tail_lds_bytes(P) == 8 * total && P.total <= TAIL_LDS_DOUBLES, "total %d, expected %ld", P.total, total);
  std::vector<std::pair<long, long>> arrays;      // [first, last + 1)
  for (int l = 0; l < nlev; l++) {
    const TailLevel &L = P.L[l];
    for (int d = 0; d < 3; d++) CHECK(L.n[d] == n[l][d] && L.e[d] == n[l][d] + 2 + kind, "level %d axis %d", l, d);
    const long arr = tail_array(L);
    arrays.push_back({ L.phi, L.phi + arr });
    if (kind == TAIL_NODES) {
      arrays.push_back({ L.tmp, L.tmp + arr });
      arrays.push_back({ L.res, L.res + arr });
      arrays.push_back({ L.sig, L.sig + (long)(L.n[0] + 2) * (L.n[1] + 2) * (L.n[2] + 2) });
    }
    // the index of the ghosted array: one-to-one
    std::vector<int> hit((size_t)arr, 0);
    for (int k = -1; k <= L.e[2] - 2; k++) for (int j = -1; j <= L.e[1] - 2; j++) for (int i = -1; i <= L.e[0] - 2; i++) {
      const int q = tail_index(L, i, j, k);
      CHECK(q >= 0 && q < arr, "level %d (%d, %d, %d): index %d of %ld", l, i, j, k, q, arr);
      if (q >= 0 && q < arr) hit[q]++;
    }
    for (long q = 0; q < arr; q++) CHECK(hit[q] == 1, "level %d: entry %ld indexed %d times", l, q, hit[q]);
  }
  if (kind == TAIL_CELLS) arrays.push_back({ P.res, P.res + (long)n[0][0] * n[0][1] * n[0][2] });
  std::sort(arrays.begin(), arrays.end());
  long end = 0;
  for (const auto &a : arrays) {
    CHECK(a.first >= end && a.second > a.first && a.second <= TAIL_LDS_DOUBLES, "array [%ld, %ld) after %ld", a.first, a.second, end);
    end = std::max(end, a.second);
  }
  CHECK(end == P.total, "arrays end at %ld, total %d", end, P.total);
}

int main() {
  static const int pers[5][3] = { { 0, 0, 0 }, { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 }, { 1, 1, 1 } };
  // the single-box hierarchies of boxes up to 64^3
  std::vector<char> owners_done(2 * 65 * 65 * 65, 0);
  for (int n0 = 1; n0 <= 64; n0++) for (int n1 = 1; n1 <= 64; n1++) for (int n2 = 1; n2 <= 64; n2++) {
    std::vector<std::array<int, 3>> lev;
    std::array<int, 3> n = { n0, n1, n2 };
    for (;;) {
      lev.push_back(n);
      bool can = true;
      for (int d = 0; d < 3; d++) if ((n[d] & 1) || n[d] <= 2) can = false;
      if (!can || lev.size() >= 31) break;
      for (int d = 0; d < 3; d++) n[d] /= 2;
    }
    for (int kind = 0; kind < 2; kind++) {
      const long most = kind == TAIL_CELLS ? 512 : 729;
      size_t first = lev.size();
      while (first > 0 && tail_points(kind, lev[first - 1].data()) <= most) first--;
      const int nl = (int)(lev.size() - first);
      if (nl < 2) continue;
      int tn[8][3] = {};
      CHECK(nl <= TAIL_MAX_LEVELS, "%d x %d x %d: %d tail levels", n0, n1, n2, nl);
      if (nl > 8) continue;
      for (int l = 0; l < nl; l++) for (int d = 0; d < 3; d++) tn[l][d] = lev[first + l][d];
      for (const auto &per : pers) check_set(kind, nl, tn, per);
      for (int l = 0; l < nl; l++) {
        char &done = owners_done[kind + 2 * (tn[l][0] + 65 * (tn[l][1] + 65 * tn[l][2]))];
        if (!done) { check_owners(kind, tn[l]); done = 1; }
      }
    }
  }
  // the extreme shapes of the point bounds: owners, and as the first of two levels where they halve
  static const int cells[3][3] = { { 1, 1, 512 }, { 2, 2, 128 }, { 8, 4, 16 } }, nodes[2][3] = { { 8, 8, 8 }, { 4, 2, 32 } };
  for (const auto &c : cells) check_owners(TAIL_CELLS, c);
  for (const auto &c : nodes) check_owners(TAIL_NODES, c);
  for (int kind = 0; kind < 2; kind++) {
    static const int sets[][2][3] = { { { 2, 2, 128 }, { 1, 1, 64 } }, { { 8, 4, 16 }, { 4, 2, 8 } }, { { 8, 8, 8 }, { 4, 4, 4 } }, { { 4, 2, 32 }, { 2, 1, 16 } },
                                      { { 1, 1, 512 }, { 1, 1, 256 } },           // does not halve
                                      { { 2, 2, 1024 }, { 1, 1, 512 } },          // too many cells
                                      { { 1, 1, 255 }, { 1, 1, 127 } },           // nodes: 1024 threads, but three 4 x 4 x 258 arrays
                                      { { 2, 2, 254 }, { 1, 1, 127 } } };         // cells: fits; nodes: too many
    for (const auto &s : sets) for (const auto &per : pers) check_set(kind, 2, s, per);
    static const int four[4][3] = { { 8, 8, 8 }, { 4, 4, 4 }, { 2, 2, 2 }, { 1, 1, 1 } };
    check_set(kind, 4, four, pers[0]);
    check_set(kind, 1, four, pers[0]);
    check_set(kind, 3, four, pers[0]);
  }
  if (g_bad) { fprintf(stderr, "%d check(s) failed\n", g_bad); return 1; }
  printf("OK %ld level sets, %ld fit\n", g_sets, g_fit);
  return 0;
}
