// vdn_switches.h -- every debug / measurement switch of the library, declared once (no HIP include: a plain C++ program can read this file).
//
// None changes a result: they select between launch forms that the tests hold bit-for-bit equal (tests/test_projection_gpu.py::
// test_multigrid_launch_variants_agree_bit_for_bit, test_kernels_gpu.py, test_amr_gpu.py) or are probes.  From the one list below come the struct
// Switches (a field per switch), its filling from the environment and the table that vdn_debug_switches() prints and vdn_init searches for
// misspelt VDN_* variables.  The code reads sw().field (runtime.hip fills the struct on first use), so a switch missing from the list does not compile.
//
// The switches exist in the TESTING build only (libvarden_amd_testing.so: -DVDN_TESTING_BUILD on runtime.hip and exchange.hip; the suite, the A/B
// tools and the one-GPU transport rehearsal load it -- VDN_LIB_FLAVOUR=testing in the Python mirror).  The shipped libvarden_amd.so reads NO
// environment variable: switches_read() hands out the defaults, every choice that matters is a field of vdn_params; vdn_init says so once if
// VDN_* switches are set.
//
// An entry: X(field, name, rule, default, doc).  The rules, e being getenv(name):
//   ON       bool    on unless atoi(e) is 0 (so "" switches off)
//   SET      bool    off unless atoi(e) is non-zero
//   PRESENT  bool    on when the variable exists at all ("=0" included)
//   INT      int     atoi(e), the default when unset
//   MIN1     int     max(1, atoi(e)), the default when unset
//   MB       size_t  atol(e) MB in bytes where that is positive, the default (bytes) otherwise
//   STR      char *  e itself (nullptr when unset)
//   LIVE     int     as INT, but read again at every sw_live() (a test sets it between two calls of one process)
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>

#define VDN_SWITCHES(X) \
  X(testing, "VDN_TESTING", STR, nullptr, "1: allows VDN_RCCL_LIB (the test transport of tests/fake_rccl); nothing else") \
  X(rccl_lib, "VDN_RCCL_LIB", STR, nullptr, "path of a library that stands in for librccl -- honoured only with VDN_TESTING=1 and the test double's handshake") \
  X(force_packed, "VDN_FORCE_PACKED", LIVE, 0, "1: box-to-box copies of one rank go through the packed per-peer buffers (device memcpy for send/recv); 2: through a 1-rank RCCL communicator (one-GPU rehearsal of the N > 1 transport)") \
  X(arena_poison, "VDN_ARENA_POISON", SET, false, "1: every byte handed back to the arena is overwritten with NaNs (a read of an entry nobody wrote fails the next solve)") \
  X(arena_chunk, "VDN_ARENA_CHUNK_MB", MB, (size_t)1024 << 20, "size of the physical chunks mapped into the arena's address range (default 1024)") \
  X(field_chunk, "VDN_FIELD_CHUNK_MB", MB, (size_t)64 << 20, "size of the pooled physical chunks behind the state fields (default 64)") \
  X(field_vmm, "VDN_FIELD_VMM", ON, true, "0: every state field is one hipMalloc block (rounds 1-5) instead of pooled chunks mapped into its own address range") \
  X(mlcc_trace, "VDN_MLCC_TRACE", SET, false, "1: the composite cell-centred solve prints its residual at every FAC iteration (stderr)") \
  X(keep_off, "VDN_KEEP_OFF", INT, 0, "mask of kept-descriptor families rebuilt at every call: 1 generic sets, 2 create_umac_grown, 4 composite cell-centred solve, 8 nodal prolongation") \
  X(sync_points, "VDN_SYNC_POINTS", INT, 0, "mask of points that synchronise the device (race hunting): 1 after every batched launch, 2 after every staged upload, 4 after every exchange, 8 before a scalar read-back, 16 at arena_reset, 32 after launch_cells") \
  X(phase_hash, "VDN_PHASE_HASH", SET, false, "1: advance_timestep prints a checksum of its fields at every phase boundary (stderr)") \
  X(no_roctx, "VDN_NO_ROCTX", PRESENT, false, "do not bind the roctx library (no bl_prof ranges)") \
  X(poll, "VDN_POLL", INT, -1, "scalar read-back: 1 spin on the pinned sequence number, 0 hipStreamSynchronize; default: spin on one rank, synchronise on several") \
  X(no_graphs, "VDN_NO_GRAPHS", PRESENT, false, "launch every multigrid cycle eagerly instead of replaying its hipGraph") \
  X(no_slope_cache, "VDN_NO_SLOPE_CACHE", PRESENT, false, "velocity mkflux recomputes the slopes of uold that velpred computed in the same step") \
  X(no_force_reuse, "VDN_NO_FORCE_REUSE", SET, false, "1: every forcing term is computed where the reference computes it (advance_premac AND velocity_advance, ...)") \
  X(slopes_march, "VDN_SLOPES_MARCH", INT, 2, "0: the per-cell slopes kernel instead of the k-marching one; 1: the march with one cell per lane and its y-neighbours from memory (kk_slopes_my); default 2: its pair form (kk_slopes_pr) wherever the layouts take it") \
  X(godunov_batch, "VDN_GODUNOV_BATCH", SET, false, "1: the descriptor (box-batched) Godunov kernels also on a level of one box") \
  X(godunov_plain, "VDN_GODUNOV_PLAIN", PRESENT, false, "the face-centred one-thread-per-cell Godunov kernels of round 1 (the fused marches' bit-for-bit reference, and their fallback where they refuse the field layouts)") \
  X(god_segw, "VDN_GOD_SEGW", ON, true, "0: the box-batched fused Godunov marches use full-width (64 x 8) tiles for every box") \
  X(god_p2, "VDN_GOD_P2", ON, true, "0: the fused marches divide by dx also where every dx is a power of two (default there: scale by 1/dx, the same doubles)") \
  X(fused_kchunks, "VDN_FUSED_KCHUNKS", MIN1, 0, "k-chunks of the fused marches (default: the count that fills the last round of workgroups best)") \
  X(god_update, "VDN_GOD_UPDATE", ON, true, "0: update_3d as its own pass instead of inside the fused mkflux march") \
  X(gsrb_pair, "VDN_GSRB_PAIR", ON, true, "0: one cell per thread in the colour passes / residuals of wide levels instead of the 2 x 2 pair form") \
  X(mac_split, "VDN_MAC_SPLIT", ON, true, "0: the finest level of macproject's one-level solve stays interleaved (kk_cc_gsrb_rho_pair) instead of stored by colour (kk_cc_gsrb_rho_split)") \
  X(mac_split_min, "VDN_MAC_SPLIT_MIN", INT, 1<<23, "fewest cells (of this rank's boxes together) of a level stored by colour (default 2^23)") \
  X(nd_rev, "VDN_ND_REV", ON, true, "0: every march of a nodal level walks its tiles in the same order (default: consecutive marches alternate)") \
  X(mac_slab, "VDN_MAC_SLAB", INT, -1, "planes per slab of the time-skewed schedule of the split level's passes (cc_split_run; default: ~200 MB of pass traffic, at most half the level); 0: whole-level launches") \
  X(mac_umax, "VDN_MAC_UMAX", ON, true, "0: max |umac| by its own pass (kk_macmax) instead of inside macproject's velocity update (kk_mkumac_rho_max)") \
  X(mac_kflip, "VDN_MAC_KFLIP", ON, true, "0: both colour passes of a sweep walk the planes upwards (default: the second colour downwards; paired and split passes of the cell-centred multigrid)") \
  X(cc_halo_faces, "VDN_CC_HALO_FACES", ON, true, "0: the cell-centred multigrid exchanges the whole ghost shell instead of the faces only") \
  X(overlap, "VDN_OVERLAP", INT, -1, "halo exchange of multigrid passes next to interior work: 1 always, 0 never, default: when a plan has a remote peer and the box is large") \
  X(mg_agglom, "VDN_MG_AGGLOM", INT, 0, "box width below which a multi-box multigrid level is gathered into one box (default: 64 across ranks, 128 where every box is this rank's)") \
  X(mg_restrict_fused, "VDN_MG_RESTRICT_FUSED", ON, true, "0: cell-centred residual and restriction as two passes") \
  X(mg_tailcycle, "VDN_MG_TAILCYCLE", ON, true, "0: the smallest levels launch by launch instead of one single-workgroup cycle") \
  X(mg_prolong_fused, "VDN_MG_PROLONG_FUSED", ON, true, "0: cell-centred prolongation as its own pass instead of inside the first post-smoothing colour pass") \
  X(mg_lds, "VDN_MG_LDS", ON, true, "0: the 16^3..64^3-cell levels of both multigrids (cell-centred and nodal) launch by launch instead of the LDS-tiled down / up kernels") \
  X(mac_stored_beta, "VDN_MAC_STORED_BETA", SET, false, "1: the finest MAC level reads stored face coefficients instead of recomputing them from rho") \
  X(mac_fast, "VDN_MAC_FAST", ON, true, "0: macproject with its rh / phi / beta multifabs as the reference has them") \
  X(hg_fast, "VDN_HG_FAST", ON, true, "0: hgproject with its rh / phi / coeffs multifabs as the reference has them") \
  X(nd_pair, "VDN_ND_PAIR", ON, true, "0: one node per lane in the nodal march instead of the pair form") \
  X(nd_lean, "VDN_ND_LEAN", ON, true, "0: whole-array zero fills of the big nodal levels instead of shell-only") \
  X(nd_restrict_fused, "VDN_ND_RESTRICT_FUSED", ON, true, "0: nodal residual and full weighting as two passes") \
  X(nd_prolong_fused, "VDN_ND_PROLONG_FUSED", ON, true, "0: nodal prolongation as a pass of its own instead of inside the first post-smoothing march") \
  X(ndf_pair, "VDN_NDF_PAIR", ON, true, "0: one node per lane in the box-batched nodal march of the composite solve") \
  X(ndm_iface_faces, "VDN_NDM_IFACE_FACES", ON, true, "0: interface interpolation of the composite nodal solve over whole boxes instead of box faces") \
  X(ndm_prolong8, "VDN_NDM_PROLONG8", ON, true, "0: correction interpolation with a thread per fine node instead of per coarse node") \
  X(ndm_neg, "VDN_NDM_NEG", SET, false, "1: the composite nodal solve copies -res into the correction's right-hand side instead of loading it directly") \
  X(fb_faces, "VDN_FB_FACES", ON, true, "0: the ghost exchanges of the composite cell-centred solve fill edges and corners too") \
  X(mlcc_rho, "VDN_MLCC_RHO", ON, true, "0: the composite MAC solve reads stored face coefficients on its finest level too") \
  X(god_narrow, "VDN_GOD_NARROW", INT, 1, "the tiling of the fused mkflux + update march of a one-box level.  0: full 64-lane tiles everywhere; 2: the remainder tile column in narrow segments (kk_mk_F_mc), no half workgroups; default 1: that, and two 256-thread workgroups per compute unit in 16-lane segments (kk_mk_F_mh) on face ranges at least 128 wide; 16 / 32: the half workgroups in segments of that many lanes on boxes of any width") \
  X(keep_sets, "VDN_KEEP_SETS", ON, true, "0: the descriptor arrays of the inter-level operators and composite solves are rebuilt and uploaded at every call") \
  X(kept_bound, "VDN_KEPT_BOUND", INT, 0, "n > 0: the kept descriptor tables hold at most n entries each (default 4096 / 64 / 512): the eviction paths in a test") \
  X(mlcc_glue, "VDN_MLCC_GLUE", ON, true, "0: the level-0 correction of the composite MAC solve stored and added in separate passes") \
  X(mlcc_fuse1, "VDN_MLCC_FUSE1", ON, true, "0: the composite MAC solve's finest-level residual and first colour pass as two launches") \
  X(batch_yz, "VDN_BATCH_YZ", ON, true, "0: no (j,k) / (i,k) tiles for thin ranges in the box-batched kernels") \
  X(batch_ppw, "VDN_BATCH_PPW", MIN1, 0, "planes per workgroup of the light box-batched kernels (default 8)") \
  X(batch_flat, "VDN_BATCH_FLAT", ON, true, "0: no flattened (i,j) plane mapping for badly filling tiles") \
  X(batch_chunk, "VDN_BATCH_CHUNK", ON, true, "0: box-batched workgroups take strided instead of contiguous plane chunks")

// per rule: the reading of e = getenv(name); what it returns is the field's type
static inline bool sw_read_ON(const char *e, bool) { return !(e && atoi(e) == 0); }
static inline bool sw_read_SET(const char *e, bool) { return e && atoi(e) != 0; }
static inline bool sw_read_PRESENT(const char *e, bool) { return e != nullptr; }
static inline int sw_read_INT(const char *e, int dflt) { return e ? atoi(e) : dflt; }
static inline int sw_read_MIN1(const char *e, int dflt) { return e ? std::max(1, atoi(e)) : dflt; }
static inline size_t sw_read_MB(const char *e, size_t dflt) { const long v = e ? atol(e) : 0; return v > 0 ? (size_t)v << 20 : dflt; }
static inline const char *sw_read_STR(const char *e, const char *) { return e; }
static inline int sw_read_LIVE(const char *e, int dflt) { return sw_read_INT(e, dflt); }

struct Switches {
#define X(field, name, rule, dflt, doc) decltype(sw_read_##rule(nullptr, dflt)) field = dflt;
  VDN_SWITCHES(X)
#undef X
};
struct SwitchInfo { const char *name, *rule, *doc; };
inline constexpr SwitchInfo switch_table[] = {
#define X(field, name, rule, dflt, doc) { name, #rule, doc },
  VDN_SWITCHES(X)
#undef X
};
// the value the environment holds for a name of the table (vdn_debug_switches prints it in both builds; nothing acts on it)
static inline const char *switch_raw(const SwitchInfo &s) { return getenv(s.name); }

// the struct as the environment sets it (testing build) or as the list's defaults do (release build: no getenv).  live_only: the LIVE entries alone
static inline void switches_read(Switches &s, bool live_only = false) {
#ifdef VDN_TESTING_BUILD
  const Switches dflt;
#define X(field, name, rule, d, doc) if (!live_only || !strcmp(#rule, "LIVE")) s.field = sw_read_##rule(getenv(name), dflt.field);
  VDN_SWITCHES(X)
#undef X
#else
  (void)s; (void)live_only;
#endif
}
