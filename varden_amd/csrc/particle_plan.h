// particle_plan.h -- the box locator of the particle module (particles.hip), host only: no HIP, no library type, so tests/cpp/particle_plan_check.cpp holds it
// without a GPU.
//
// On one level, every box face lies on a multiple of some block size from the domain's low corner: blk[d] is the LARGEST such size, the gcd of every box's
// lo - pd.lo, hi + 1 - pd.lo and of the domain extent along d (the grid generator's blocking factor makes it 4 or more on real hierarchies; 1 is legal).  The level's
// domain is then n[0] x n[1] x n[2] blocks, no block is cut by a box face, and ONE int32 per block -- the global index of the box that holds it, or -1 -- finds the
// box of a cell with three divisions and one load, whatever the number of boxes.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

constexpr long PARTICLE_MAP_CAP = 1L << 25;      // entries of one level's map (128 MiB of int32): a level that needs more is refused

struct ParticleMap {
  int lo[3] = {0, 0, 0}, hi[3] = {-1, -1, -1};   // the level's domain, in cells
  int blk[3] = {1, 1, 1}, n[3] = {0, 0, 0};      // block size and number of blocks per direction
  std::vector<int32_t> box;                       // [(k * n[1] + j) * n[0] + i] -> global box index or -1
};

inline int particle_gcd(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a < 0 ? -a : a; }

// the entry of cell c (inside the domain) in a map of block size blk and n blocks per direction over a domain whose low corner is lo
#if defined(__HIPCC__)
__host__ __device__
#endif
inline long particle_map_index(const int c[3], const int lo[3], const int blk[3], const int n[3]) {
  return ((long)((c[2] - lo[2]) / blk[2]) * n[1] + (c[1] - lo[1]) / blk[1]) * n[0] + (c[0] - lo[0]) / blk[0];
}

// builds the map of level `lev` (the number only names the level in a refusal) from its GLOBAL box list; B: anything with int lo[3], hi[3].
// Returns an empty string, or the reason of the refusal: a box outside the domain, two boxes on one block, or more than PARTICLE_MAP_CAP entries.
template <class B>
inline std::string particle_plan(int lev, const std::vector<B> &boxes, const B &pd, ParticleMap *out) {
  ParticleMap M;
  char msg[256];
  for (int d = 0; d < 3; d++) {
    M.lo[d] = pd.lo[d]; M.hi[d] = pd.hi[d];
    const int ext = pd.hi[d] - pd.lo[d] + 1;
    if (ext < 1) { snprintf(msg, sizeof msg, "level %d: the domain is empty along direction %d", lev, d); return msg; }
    int g = ext;
    for (const B &b : boxes) {
      if (b.lo[d] < pd.lo[d] || b.hi[d] > pd.hi[d] || b.hi[d] < b.lo[d]) { snprintf(msg, sizeof msg, "level %d: a box lies outside the domain along direction %d", lev, d); return msg; }
      g = particle_gcd(g, b.lo[d] - pd.lo[d]);
      g = particle_gcd(g, b.hi[d] + 1 - pd.lo[d]);
    }
    M.blk[d] = g; M.n[d] = ext / g;
  }
  const long total = (long)M.n[0] * M.n[1] * M.n[2];
  if (total > PARTICLE_MAP_CAP) {
    snprintf(msg, sizeof msg, "level %d: the box locator needs %ld entries at block size %d x %d x %d, more than the %ld it may hold", lev, total, M.blk[0], M.blk[1],
             M.blk[2], PARTICLE_MAP_CAP);
    return msg;
  }
  M.box.assign((size_t)total, -1);
  for (int q = 0; q < (int)boxes.size(); q++) {
    const B &b = boxes[q];
    int a[3], z[3];
    for (int d = 0; d < 3; d++) { a[d] = (b.lo[d] - M.lo[d]) / M.blk[d]; z[d] = (b.hi[d] - M.lo[d]) / M.blk[d]; }
    for (int k = a[2]; k <= z[2]; k++) for (int j = a[1]; j <= z[1]; j++) for (int i = a[0]; i <= z[0]; i++) {
      int32_t &e = M.box[((size_t)k * M.n[1] + j) * M.n[0] + i];
      if (e != -1) { snprintf(msg, sizeof msg, "level %d: boxes %d and %d overlap", lev, (int)e, q); return msg; }
      e = q;
    }
  }
  *out = std::move(M);
  return std::string();
}
