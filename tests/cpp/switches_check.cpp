// The reading rules of varden_amd/csrc/vdn_switches.h, without a GPU and without the library: one switch of each rule is set to nothing, "", "0", "1"
// and "7", the struct is read again, and the field is held against the rule as the accessors had it before the list existed (env_on: on unless atoi
// gives 0; env_set: off unless non-zero; "present at all"; env_int: atoi or the default; max(1, atoi); a positive count of MB or the default).
// Built twice by tests/test_switches_cpu.py: with -DVDN_TESTING_BUILD (the rules) and without (the release build: the defaults, whatever is set).
#include "vdn_switches.h"
#include <cstdio>
#include <set>
#include <string>

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_bad++; fprintf(stderr, "FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)

static const char *const VALUES[5] = { nullptr, "", "0", "1", "7" };
static void put(const char *name, const char *v) { if (v) setenv(name, v, 1); else unsetenv(name); }
static void clear_all() { for (const SwitchInfo &s : switch_table) unsetenv(s.name); }
static bool same(const Switches &a, const Switches &b) {
  bool eq = true;
#define X(field, name, rule, dflt, doc) eq = eq && a.field == b.field;
  VDN_SWITCHES(X)
#undef X
  return eq;
}

int main() {
  const Switches dflt;
  // the table: an entry per field, no name twice, every name a VDN_ one
  std::set<std::string> names;
  for (const SwitchInfo &s : switch_table) { names.insert(s.name); CHECK(std::string(s.name).rfind("VDN_", 0) == 0 && s.doc[0] && s.rule[0], "%s", s.name); }
  CHECK(names.size() == sizeof switch_table / sizeof switch_table[0] && names.size() == 59, "%zu names", names.size());
  // the defaults the code had at its use sites
  CHECK(dflt.mac_split && !dflt.phase_hash && !dflt.no_graphs && dflt.overlap == -1 && dflt.batch_ppw == 0 && dflt.fused_kchunks == 0, "defaults");
  CHECK(dflt.mac_split_min == 1 << 23 && dflt.mac_slab == -1 && dflt.poll == -1 && dflt.mg_agglom == 0 && dflt.kept_bound == 0 && dflt.force_packed == 0, "defaults");
  CHECK(dflt.arena_chunk == (size_t)1024 << 20 && dflt.field_chunk == (size_t)64 << 20 && !dflt.rccl_lib && !dflt.testing && !dflt.mac_stored_beta, "defaults");
  clear_all();
  Switches s;
  switches_read(s);
  CHECK(same(s, dflt), "an empty environment gives the defaults");
#ifdef VDN_TESTING_BUILD
  //                              unset          ""     "0"    "1"          "7"
  const bool   on[5]      = { true,          false, false, true,        true };               // env_on: VDN_MAC_SPLIT
  const bool   set[5]     = { false,         false, false, true,        true };               // env_set: VDN_PHASE_HASH
  const bool   present[5] = { false,         true,  true,  true,        true };               // getenv != nullptr: VDN_NO_GRAPHS (=0 still disables graphs)
  const int    integer[5] = { -1,            0,     0,     1,           7 };                  // env_int(name, -1): VDN_OVERLAP
  const int    min1[5]    = { 0,             1,     1,     1,           7 };                  // max(1, atoi), 0 = unset: VDN_BATCH_PPW (=0 gives 1)
  const size_t mb[5]      = { (size_t)64 << 20, (size_t)64 << 20, (size_t)64 << 20, (size_t)1 << 20, (size_t)7 << 20 };      // env_mb(name, 64): VDN_FIELD_CHUNK_MB
  const int    live[5]    = { 0,             0,     0,     1,           7 };                  // atoi or 0: VDN_FORCE_PACKED
  for (int i = 0; i < 5; i++) {
    const char *v = VALUES[i], *what = v ? v : "(unset)";
    for (const char *n : { "VDN_MAC_SPLIT", "VDN_PHASE_HASH", "VDN_NO_GRAPHS", "VDN_OVERLAP", "VDN_BATCH_PPW", "VDN_FIELD_CHUNK_MB", "VDN_FORCE_PACKED", "VDN_RCCL_LIB" }) put(n, v);
    Switches r;
    switches_read(r);
    CHECK(r.mac_split == on[i], "VDN_MAC_SPLIT=%s", what);
    CHECK(r.phase_hash == set[i], "VDN_PHASE_HASH=%s", what);
    CHECK(r.no_graphs == present[i], "VDN_NO_GRAPHS=%s", what);
    CHECK(r.overlap == integer[i], "VDN_OVERLAP=%s gives %d", what, r.overlap);
    CHECK(r.batch_ppw == min1[i], "VDN_BATCH_PPW=%s gives %d", what, r.batch_ppw);
    CHECK(r.field_chunk == mb[i], "VDN_FIELD_CHUNK_MB=%s gives %zu", what, r.field_chunk);
    CHECK(r.force_packed == live[i], "VDN_FORCE_PACKED=%s gives %d", what, r.force_packed);
    CHECK(v ? (r.rccl_lib && std::string(r.rccl_lib) == v) : !r.rccl_lib, "VDN_RCCL_LIB=%s", what);
    // every other field keeps its default
    Switches q = r;
    q.mac_split = dflt.mac_split; q.phase_hash = dflt.phase_hash; q.no_graphs = dflt.no_graphs; q.overlap = dflt.overlap; q.batch_ppw = dflt.batch_ppw;
    q.field_chunk = dflt.field_chunk; q.force_packed = dflt.force_packed; q.rccl_lib = dflt.rccl_lib;
    CHECK(same(q, dflt), "fields of switches that are not set moved (%s)", what);
  }
  // the second switch of the max(1, atoi) rule, and a negative count of MB
  put("VDN_FUSED_KCHUNKS", "0"); put("VDN_ARENA_CHUNK_MB", "-3");
  switches_read(s);
  CHECK(s.fused_kchunks == 1 && s.arena_chunk == dflt.arena_chunk, "VDN_FUSED_KCHUNKS=0 gives %d", s.fused_kchunks);
  // a LIVE entry is read again by a live-only pass, a cached one is not
  clear_all();
  switches_read(s);
  put("VDN_FORCE_PACKED", "2"); put("VDN_MAC_SPLIT", "0");
  switches_read(s, true);
  CHECK(s.force_packed == 2 && s.mac_split, "live-only pass: force_packed %d mac_split %d", s.force_packed, (int)s.mac_split);
#else
  // the release build: every one of those variables set, and the struct still holds the defaults
  for (const char *v : VALUES) {
    for (const SwitchInfo &t : switch_table) put(t.name, v);
    Switches r;
    switches_read(r);
    CHECK(same(r, dflt), "the release build read a switch (%s)", v ? v : "(unset)");
    switches_read(r, true);
    CHECK(same(r, dflt), "the release build read a live switch (%s)", v ? v : "(unset)");
  }
#endif
  if (!g_bad) printf("OK\n");
  return g_bad ? 1 : 0;
}
