// nd_lds_plan.h -- the tile arithmetic of the nodal multigrid's LDS-tiled levels (kk_nd_lds_down / kk_nd_lds_up in mg_nd.hip): which nodes a workgroup owns,
// on which nodes it runs the two pre-smoothing sweeps and the residual with redundant halo work, and which levels take this form at all.  Integers only: no HIP,
// no ctx(), no sw() -- the kernels and the host read it, and so does tests/cpp/nd_lds_plan_check.cpp with a host compiler.
//
// A level of n cells per axis (n a multiple of 8) has nodes 0 .. n.  Tile a of n / 8 owns the fine nodes 8a .. 8a+7 and the coarse nodes 4a .. 4a+3 under them;
// the last tile of an axis also owns node n and coarse node n / 2.  All ranges below are inclusive and NOT yet clipped to 0 .. n: nodes outside the level hold zero.
#pragma once
#if defined(__HIPCC__)
#define ND_LDS_FN __host__ __device__ inline
#else
#define ND_LDS_FN inline
#endif

#define ND_LDS_T 8            // fine nodes a tile owns per axis (the last one: 9)
#define ND_LDS_NMIN 16        // extents (cells) of a level that takes the tiled form: multiples of ND_LDS_T in ND_LDS_NMIN .. ND_LDS_NMAX
#define ND_LDS_NMAX 64
#define ND_LDS_BOX 13         // the down kernel's phi box per axis: nodes 8a-3 .. 8a+9 (sweep 1's region; the residual of nodes 8a-1 .. 8a+9 is kept in the same box)
#define ND_LDS_SIG 14         // ... and its sigma box: cells 8a-4 .. 8a+9
#define ND_LDS_UBOX 11        // the up kernel's phi box: nodes 8a-1 .. 8a+9
#define ND_LDS_USIG 10        // ... and its sigma box: cells 8a-1 .. 8a+8

struct NdLdsRange { int lo, hi; };

// the refusal rule for one extent
ND_LDS_FN bool nd_lds_extent_ok(int n) { return n % ND_LDS_T == 0 && n >= ND_LDS_NMIN && n <= ND_LDS_NMAX; }
ND_LDS_FN int nd_lds_tiles(int n) { return n / ND_LDS_T; }
ND_LDS_FN bool nd_lds_last(int n, int a) { return a == n / ND_LDS_T - 1; }
// owned: written by this tile and by no other
ND_LDS_FN NdLdsRange nd_lds_own_fine(int n, int a) { return NdLdsRange{ ND_LDS_T * a, nd_lds_last(n, a) ? n : ND_LDS_T * a + ND_LDS_T - 1 }; }
ND_LDS_FN NdLdsRange nd_lds_own_coarse(int n, int a) { return NdLdsRange{ (ND_LDS_T / 2) * a, nd_lds_last(n, a) ? n / 2 : (ND_LDS_T / 2) * a + ND_LDS_T / 2 - 1 }; }
// the boxes held in LDS (first node / cell and ND_LDS_* entries per axis)
ND_LDS_FN int nd_lds_box_lo(int a) { return ND_LDS_T * a - 3; }
ND_LDS_FN int nd_lds_sig_lo(int a) { return ND_LDS_T * a - 4; }
ND_LDS_FN int nd_lds_ubox_lo(int a) { return ND_LDS_T * a - 1; }
ND_LDS_FN int nd_lds_usig_lo(int a) { return ND_LDS_T * a - 1; }
// the three working regions of the down kernel: sweep 1 (from phi = 0: reads no phi), sweep 2 (reads sweep 1 one node around), the residual (reads sweep 2 one
// node around; what the full weighting of the owned coarse nodes reads, 8a-1 .. 8a+7 and one more where the tile owns coarse node n / 2)
ND_LDS_FN NdLdsRange nd_lds_sweep1(int a) { return NdLdsRange{ ND_LDS_T * a - 3, ND_LDS_T * a + 9 }; }
ND_LDS_FN NdLdsRange nd_lds_sweep2(int a) { return NdLdsRange{ ND_LDS_T * a - 2, ND_LDS_T * a + 8 }; }
ND_LDS_FN NdLdsRange nd_lds_resid(int n, int a) { return NdLdsRange{ ND_LDS_T * a - 1, nd_lds_last(n, a) ? ND_LDS_T * a + 8 : ND_LDS_T * a + 7 }; }
// the residual entries the kernel stores (zeros beyond the residual's region): what nd_fw27 around the owned coarse nodes may read
ND_LDS_FN NdLdsRange nd_lds_resbox(int a) { return NdLdsRange{ ND_LDS_T * a - 1, ND_LDS_T * a + 9 }; }
