/*
 * varden_amd.h -- C-ABI of the MI355X-native VARDEN hot path.
 *
 * This is the drop-in boundary for the reference's per-timestep path
 *     advance_module::advance_timestep      (reference src/advance_timestep.f90:26-44)
 *     estdt_module::estdt                   (reference src/estdt.f90:15)
 *     hgproject_module::hgproject           (reference src/hgproject.f90:17-18, called by the
 *                                            driver for the initial projection, varden.f90:134)
 * and for the BoxLib (FBoxLib, external to the reference tree) containers those
 * routines take: box / ml_layout / multifab / bc_tower.  A Fortran ISO_C_BINDING
 * module that re-exports these entry points under the BoxLib names lives in
 * varden_amd/fortran/varden_amd_mod.f90; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; the message is
 *     available from vdn_last_error() (reference: bl_error aborts; the Fortran
 *     shim turns non-zero into `error stop`).  A HIP error the CALLER left pending on the
 *     calling thread is cleared at entry (noted once per process on stderr) and not restored
 *     -- HIP offers no way to put it back --: every entry point then reports any launch
 *     failure of its own, whatever its code.  A host that polls hipGetLastError() after
 *     calling in asks vdn_last_stale_hip_error() for what was taken off its thread.
 *   - plain pointers and sizes only.  "device" pointers are hipMalloc'ed HBM.
 *   - all floating point data is IEEE f64; arrays use the BoxLib fab layout:
 *         p(lo1-ng:hi1+ng[+nodal1], lo2-ng:..., lo3-ng:..., 1:nc)   column-major,
 *     x fastest, component slowest (reference evidence: src/mkflux.f90:74-92).
 *   - indices (lo/hi) are 0-based cell indices of the level's index space, as in
 *     BoxLib; direction index d = 0,1,2 ; side 0 = lo, 1 = hi.
 */
#ifndef VARDEN_AMD_H
#define VARDEN_AMD_H
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- bc_module constants (FBoxLib values; reference use: src/define_bc_tower.f90:199-335,
 *      exec/test/inputs_*: -1 periodic, 11 inlet, 12 outlet, 14 slip, 15 no-slip) -------- */
enum {
  VDN_PERIODIC = -1, VDN_INTERIOR = 0, VDN_INLET = 11, VDN_OUTLET = 12, VDN_SYMMETRY = 13,
  VDN_SLIP_WALL = 14, VDN_NO_SLIP_WALL = 15,
  VDN_REFLECT_ODD = 20, VDN_REFLECT_EVEN = 21, VDN_FOEXTRAP = 22, VDN_EXT_DIR = 23, VDN_HOEXTRAP = 24,
  VDN_BC_PER = -1, VDN_BC_INT = 0, VDN_BC_DIR = 1, VDN_BC_NEU = 2
};

/* ---- proj_parameters (reference src/proj_parameters.f90:5-8) ------------------------------ */
enum { VDN_INITIAL_PROJECTION = 1, VDN_DIVU_ITERS = 2, VDN_PRESSURE_ITERS = 3, VDN_REGULAR_TIMESTEP = 4 };

/* ---- runtime parameters read implicitly by the reference kernels through probin_module
 *      (reference src/_parameters, src/probin.template).  One POD passed once. ------------- */
typedef struct vdn_params {
  int    dm;              /* dim_in: 3, or 2 (one level, any list of boxes, any ranks)          */
  int    nscal;           /* nscal (2): the density and nscal-1 passive tracers; 1..11        */
                          /* (nscal+5 <= 16 bc components; vdn_init refuses others)           */
  int    slope_order;     /* 0, 2 or 4 (default 4)                                            */
  int    use_minion;      /* logical use_minion (default 0)                                   */
  int    boussinesq;      /* default 0                                                        */
  int    stencil_order;   /* 2                                                                */
  int    diffusion_type;  /* 1 = Crank-Nicolson, 2 = backward Euler                           */
  int    verbose;
  int    mg_verbose;
  int    prob_type;       /* only used for the hgproject abs-eps special case (prob_type 4)   */
  double visc_coef;       /* >= 0; > 0 enables the viscous solve (viscsolve.f90:19-306)          */
  double diff_coef;       /* >= 0; > 0 enables diff_scalar_solve (viscsolve.f90:308-515)        */
  double cflfac;          /* 0.8                                                              */
  double max_dt_growth;   /* 1.1                                                              */
  /* inflow data used by multifab_physbc EXT_DIR fills: [dir][side]                           */
  double u_bc[3][2], v_bc[3][2], w_bc[3][2], rho_bc[3][2], trac_bc[3][2];
  /* multigrid controls (the solvers are external to the reference tree; these are ours)      */
  int    mg_nu1, mg_nu2;          /* pre/post smoothing sweeps (2,2)                          */
  int    mg_nub;                  /* bottom sweeps on the coarsest level                      */
  int    mg_max_iter;             /* max V-cycles for the MAC solve (100)                     */
  int    hg_max_iter;             /* max V-cycles for the nodal solve (reference: 100)        */
  int    hg_nu1, hg_nu2, hg_nub;
  double hg_omega;                /* nodal Jacobi damping                                     */
  double mac_rel_eps;             /* 1e-10: reference src/macproject.f90:91-93                */
  double hg_rel_eps;              /* <=0: use 1e-12/1e-11/1e-10 by nlevs, hgproject.f90:113-119 */
  int    abort_on_max_iter;       /* 1 (default): a solve that reaches its iteration cap or meets a non-finite norm fails the call,
                                   * as FBoxLib's solvers abort (bl_error); 0: report through vdn_last_solver_stats and go on */
  int    hg_fmg;                  /* 1 (default): a nodal solve that starts from phi = 0 takes its initial guess from a nested iteration
                                   * (right-hand side restricted down, one V-cycle per level on the way up): two V-cycles fewer at 1e-12;
                                   * 0: V-cycles from the zero guess (rounds 1 and 2)                                              */
  int    mac_fmg;                 /* 1 (default): the same for the cell-centred solve of the MAC projection (whose phi starts from zero):
                                   * right-hand side averaged down to the coarsest level of at least 16^3 cells, two V-cycles there, then
                                   * per level a linear interpolation of the solution and one V-cycle; one V-cycle fewer at 1e-10; 0: off */
  double hg_omega_pre1, hg_omega_pre2;   /* 1.45, 0.7 (adjacent in memory, in this order): with hg_nu1 = 2 the two pre-smoothing sweeps of the nodal V-cycle
                                   * are damped by these instead of hg_omega -- a two-step Chebyshev pair, one V-cycle fewer at 256^3; either <= 0: hg_omega */
  double hg_omega_fac1, hg_omega_fac2, hg_omega_fac3;   /* 1.6, 0.9, 0.65: with hg_nu1 + hg_nu2 = 3 the three relaxation sweeps on a refined level of the
                                   * composite nodal solve (nlevs > 1) are damped by these -- a three-step Chebyshev set; any <= 0: hg_omega */
  int    mg_predict;              /* 1 (default): a projection's multigrid (one level, zero initial guess) does not read its residual norm back before the
                                   * cycle at which the previous solve of the same size stopped, minus one: the norms of the cycles in between are kept on the
                                   * device and read in one go (one read-back -- at N > 1 one all-reduce -- instead of one per V-cycle).  The stopping cycle is
                                   * decided by the same norms: if the history shows an earlier cycle had already converged, the solve is REPEATED with a
                                   * read-back per cycle, so results never depend on the prediction; 0: read every cycle (rounds 1-3) */
  /* Bottom solvers of the two multigrids (reference src/_parameters:55-57, handed to ml_cc_solve / ml_nd_solve in mac_multigrid.f90:56-58 and
   * hg_multigrid.f90:99-100).  mg_bottom_solver governs EVERY cell-centred solve (the MAC projection, the viscous and the scalar diffusion solves: the
   * reference routes them all through mac_multigrid), hg_bottom_solver the nodal one.  Values -- the numbering is FBoxLib's as published, which is not
   * in the reference tree (EXT-UNVERIFIED):
   *   -1 (default), 0, 4: the bottom sweeps -- max(mg_nub, N^2) red-black Gauss-Seidel / max(hg_nub, 2 N^2) Jacobi sweeps, N the bottom level's largest
   *                 extent.  -1 is this library's default; 4 asks for an agglomerated multigrid at the bottom, which the replicated tail already is.
   *   1, 3:         BiCGStab (3 is FBoxLib's communication-avoiding variant: it differs in communication only, and one workgroup has none).
   *   2:            conjugate gradients.
   *   anything else: vdn_init fails.
   * Both Krylov methods are preconditioned by the operator's diagonal, start from zero, stop when the max-norm of the residual has fallen by
   * *_bottom_solver_eps relative to the bottom right-hand side, and are capped at 12 N iterations.  A bottom level of fewer than 4913 = 17^3 points (cells, or
   * nodes) is solved by ONE workgroup in one launch (csrc/krylov_wg.h); a larger one -- 75^3 cells under n_cell = 150 or 300, 125^3 under 250 or 500 -- by
   * the whole GPU, the same iteration as a fixed sequence of plain launches per visit (csrc/krylov_grid.h; dm = 3 only; vdn_last_bottom_form tells which).
   * A breakdown (rho or omega zero or not
   * finite, p.Ap <= 0) leaves the last iterate, is counted (vdn_last_bottom_stats) and the V-cycle goes on.  They apply where one rank holds the whole
   * bottom level: the last level of a one-box hierarchy and of the replicated tail (any boxes, any ranks; level 0 of a composite solve included), and
   * the last level of both dm = 2 multigrids (any boxes, any ranks: they work on a gathered level that every rank holds whole).  A bottom level still
   * distributed over boxes keeps its sweeps, and so does a hierarchy of ONE level (an odd extent on the finest level, in dm = 2 and dm = 3 alike), which
   * reports zero statistics.  With -1, 0 or 4 no launch and no bit differs from before. */
  int    mg_bottom_solver, hg_bottom_solver;
  int    max_mg_bottom_nlevels;   /* 1000 (src/_parameters:57): carried for the reference's namelist; NO effect (the levels under the bottom are the replicated tail) */
  double mg_bottom_solver_eps;    /* 1e-3: mac_multigrid.f90:56 (bottom_solver_eps = 1.d-3) */
  double hg_bottom_solver_eps;    /* 1e-3: OURS -- hg_multigrid.f90 passes none and FBoxLib's default is not in the reference tree */
} vdn_params;

/* fills *p with the reference defaults (src/_parameters) */
void vdn_params_default(vdn_params *p);

typedef struct vdn_box { int lo[3]; int hi[3]; } vdn_box;

typedef struct vdn_layout   vdn_layout;    /* ml_layout (+ per-level layout, box->rank map)    */
typedef struct vdn_multifab vdn_multifab;  /* multifab of one level                            */
typedef struct vdn_bc_tower vdn_bc_tower;  /* define_bc_module::bc_tower                       */

/* ------------------------------------------------------------------------------------------- */
/* runtime                                                                                     */
/* ------------------------------------------------------------------------------------------- */
int  vdn_init(const vdn_params *prm, int rank, int nranks, int device);
/* Debug / measurement switches.  The library reads environment variables VDN_* only through one list (varden_amd/csrc/vdn_switches.h: name, reading rule, default
 * and meaning of each, read once per process into one struct): each selects between launch forms that the test suite holds bit-for-bit equal, or is a probe; none changes a result, none is needed in production.  This call
 * returns the table as text -- one line per switch: name, current value, what it does.  vdn_init warns on stderr about VDN_* variables that are not in it.
 * Groups: transport rehearsal (VDN_FORCE_PACKED, VDN_RCCL_LIB + VDN_TESTING); runtime (VDN_ARENA_POISON, VDN_POLL, VDN_NO_GRAPHS,
 * VDN_NO_ROCTX, VDN_KEEP_SETS, VDN_KEPT_BOUND); advance (VDN_NO_SLOPE_CACHE, VDN_NO_FORCE_REUSE); Godunov launch forms (VDN_GOD_*, VDN_GODUNOV_*, VDN_SLOPES_MARCH,
 * VDN_FUSED_KCHUNKS); cell-centred multigrid (VDN_GSRB_PAIR, VDN_CC_HALO_FACES, VDN_MG_*, VDN_MAC_*, VDN_OVERLAP*); nodal
 * multigrid (VDN_ND_*, VDN_HG_FAST, and VDN_MG_LDS, which both multigrids read: their 16^3..64^3-cell levels launch by launch); composite solves (VDN_NDF_*, VDN_NDM_*, VDN_MLCC_*, VDN_FB_FACES); box-batched kernels (VDN_BATCH_*). */
const char *vdn_debug_switches(void);
/* "release": libvarden_amd.so -- reads NO environment variable (the switches are compiled out, RCCL is the only transport); "testing": libvarden_amd_testing.so,
 * the same objects with the switch table and the test-transport seam compiled in (the test suite, the A/B tools, the one-GPU transport rehearsal).
 * The testing build alone also exports `unsigned vdn_nd_prolong_fused_levels(void)`: bit l is set when level l of the last nodal solve took its coarse
 * correction inside the first post-smoothing march (the read-back of tests/test_nd_prolong_fused_gpu.py; not part of the product's interface), and
 * `unsigned vdn_nd_lds_levels(void)`: bit l is set when level l of the last nodal solve ran as one launch down and one up (tests/test_nd_lds_levels_gpu.py), and
 * `int vdn_last_tail_form(int which)`: the body the last one-workgroup tail cycle of a cell-centred (which = 0) or the nodal (1) solve took, 0: on global memory,
 * 1: levels in LDS (tests/test_tail_cycles_gpu.py), and `int vdn_last_slopes_form(void)`: the form the last slope launch of velpred / mkflux took, 0: one thread
 * per cell, 1: the k-march with one cell per lane, 2: its pair form (tests/test_slopes_march_gpu.py), and `int vdn_last_mkflux_form(void)`: the family of the last
 * one-box mkflux march, 0: kk_mk_F_m, 1: kk_mk_F_mc, 16 / 32: kk_mk_F_mh in segments of that many lanes (tests/test_godunov_half_gpu.py). */
const char *vdn_build_flavour(void);
int  vdn_finalize(void);
const char *vdn_last_error(void);
/* the hipError_t (as int; 0 = none) most recently found pending at the entry of a call and cleared there (see Conventions); clear != 0 resets it */
int  vdn_last_stale_hip_error(int clear);
/* Launch stream.  Default: a PRIVATE non-blocking stream created by vdn_init -- not ordered against the legacy null stream or any
 * stream of the host application.  Calls that only enqueue work (setval, copy_c, fill_boundary, physbc, the vdn_k_* hooks) return
 * before it has run; vdn_multifab_dataptr drains the private stream before handing a device pointer out, vdn_device_synchronize
 * drains it on request.  vdn_set_stream(s) makes every launch go to the caller's stream s instead (the caller then orders its own work
 * on s; nothing is drained for it); vdn_set_stream(NULL) returns to the private stream. */
int  vdn_set_stream(void *hip_stream);
int  vdn_device_synchronize(void);
/* arena of per-step temporaries (the multifabs advance_timestep.f90:65-80 allocates and frees every step): bytes backed by device memory (1 GB chunks mapped
 * into a reserved address range as the high-water mark moves), high-water mark */
int  vdn_arena_stats(size_t *reserved_bytes, size_t *peak_bytes);
/* A 2-D problem run as its z-uniform, z-periodic 3-D copy (the hierarchies of the reference's 2-D inputs: varden_amd/driver.py, VardenAMR(extrude2d = nz)): with
 * w = 0 and nothing varying along z the 3-D scheme IS the 2-D one -- velpred_3d / mkflux_3d reduce to velpred_2d / mkflux_2d, the 7-point and 27-point operators to
 * the 5-point and 9-point ones -- except where the reference's two restatements differ: velpred_3d clamps the normal velocity of a hi-x OUTLET face with min()
 * (src/velpred.f90:2075), velpred_2d with max() (:305).  on != 0 selects velpred_2d's rule in the 3-D kernels.  Default 0; reset by vdn_init. */
int  vdn_set_extruded_2d(int on);
int  vdn_get_params(vdn_params *out);

/* ------------------------------------------------------------------------------------------- */
/* rank-to-rank transport (replaces FBoxLib's `parallel` MPI wrapper on the hot path): one rank  */
/* per GPU, RCCL point-to-point for ghost exchange, ncclAllReduce(MAX) for norms / estdt.          */
/* Rank 0 calls vdn_comm_get_unique_id, the host broadcasts the 128 bytes (MPI_Bcast in a Fortran   */
/* driver, torch.distributed in bench.py), every rank calls vdn_comm_init.  No-ops when nranks = 1. */
/* ------------------------------------------------------------------------------------------- */
int  vdn_comm_get_unique_id(char *id128);
int  vdn_comm_init(const char *id128);
int  vdn_comm_finalize(void);
/* ranks of the live RCCL communicator (ncclCommCount); 1 when none is up -- bench.py reports it as rccl_nranks */
int  vdn_comm_nranks(int *n);
/* MAX over the ranks of n host doubles, in place (parallel_reduce(..., MPI_MAX) of a Fortran driver; the file writers use it for the
 * per-box minima / maxima and as their barrier).  No-op when nranks = 1. */
int  vdn_comm_allreduce_max(double *host, int n);
/* traffic counters since the last reset (24 longs): [0] ghost exchanges with remote traffic (pack + one ncclGroup + unpack each),
 * [1] ncclSend calls, [2] doubles sent, [3] all-reduces, [4] all-gathers, [5] doubles contributed to them, [6] refreshes of
 * inter-level views, [7] doubles they sent, [8+b] exchanges that sent [2^(10+b), 2^(11+b)) bytes.  The exchange sites of the reference:
 * src/velpred.f90:102-119, src/macproject.f90:117,492, src/estdt.f90:69; everything inside ml_cc_solve / ml_nd_solve is FBoxLib's. */
int  vdn_comm_stats(long *out24, int reset);
/* "rccl", "test-double" (tests/fake_rccl, only with VDN_TESTING=1 -- see exchange.hip) or "none" (no transport loaded: one rank) */
const char *vdn_comm_transport(void);
/* host-only introspection of the ghost-exchange plan (used by the CPU multi-process tests): the remote  */
/* copies rank `as_rank` performs for a multifab (nc, ng, nodal) on the given boxes; rows of 14 longs:  */
/* [kind 0=send 1=recv, peer, lo[3], hi[3], shift[3], buffer offset (doubles), dst box, src box]          */
int  vdn_plan_describe(const vdn_box *pd, const int *pmask, int nboxes, const vdn_box *boxes, const int *owner,
                       int nc, int ng, const int *nodal, int as_rank, long *rows, int maxrows,
                       int *nrows, int *nlocal_descs);
/* host-only introspection of the box index behind the box-pair loops of the inter-level operators (CPU tests): the boxes of the list that the  */
/* index names as candidates for touching [qlo - margin, qhi + margin], ascending; *ncand their number (out holds the first maxout)            */
int  vdn_box_candidates(int nboxes, const vdn_box *boxes, const int *qlo, const int *qhi, int margin, int *out, int maxout, int *ncand);

/* ------------------------------------------------------------------------------------------- */
/* ml_layout: nlev levels; rr[nlev-1][3] refinement ratios; pd[nlev] problem domains;          */
/* boxes of all levels concatenated (nboxes[l] each); owner[] = rank of each box;              */
/* pmask[3] periodicity.  (BoxLib: ml_layout_build / layout_build_ba)                          */
/* ------------------------------------------------------------------------------------------- */
int  vdn_layout_create(int nlev, const int *rr, const vdn_box *pd, const int *nboxes,
                       const vdn_box *boxes, const int *owner, const int *pmask, vdn_layout **out);
int  vdn_layout_destroy(vdn_layout *la);
int  vdn_layout_nlevel(const vdn_layout *la);
int  vdn_layout_nboxes(const vdn_layout *la, int lev);          /* global number of boxes     */
int  vdn_layout_nlocal(const vdn_layout *la, int lev);          /* boxes owned by this rank    */
int  vdn_layout_global_index(const vdn_layout *la, int lev, int local_i);
int  vdn_layout_get_box(const vdn_layout *la, int lev, int global_i, vdn_box *out);

/* ------------------------------------------------------------------------------------------- */
/* bc_tower: built from the domain phys_bc[dir][side] exactly as define_bc_tower.f90 does       */
/* (phys 129-156, adv 158-252, ell 254-340).  Arrays are addressed [grid][dir][side][comp]      */
/* with grid 0 = whole domain, grids 1..nlocal = local boxes, comp 0-based.                     */
/* ------------------------------------------------------------------------------------------- */
int  vdn_bc_tower_create(const vdn_layout *la, const int *phys_bc /*[3][2]*/, vdn_bc_tower **out);
int  vdn_bc_tower_destroy(vdn_bc_tower *bct);
int  vdn_bc_tower_phys(const vdn_bc_tower *b, int lev, int grid, int dir, int side);
int  vdn_bc_tower_adv (const vdn_bc_tower *b, int lev, int grid, int dir, int side, int comp);
int  vdn_bc_tower_ell (const vdn_bc_tower *b, int lev, int grid, int dir, int side, int comp);

/* ------------------------------------------------------------------------------------------- */
/* multifab (BoxLib multifab_module names in comments)                                          */
/* ------------------------------------------------------------------------------------------- */
int  vdn_multifab_create(const vdn_layout *la, int lev, int nc, int ng, const int *nodal /*[3] or NULL*/,
                         vdn_multifab **out);                                   /* multifab_build[_edge] */
int  vdn_multifab_destroy(vdn_multifab *mf);                                    /* multifab_destroy      */
int  vdn_multifab_nfabs(const vdn_multifab *mf);                                /* nfabs                 */
int  vdn_multifab_ncomp(const vdn_multifab *mf);
int  vdn_multifab_nghost(const vdn_multifab *mf);
int  vdn_multifab_get_box(const vdn_multifab *mf, int local_i, vdn_box *out);   /* get_box (valid cells) */
long vdn_multifab_fab_size(const vdn_multifab *mf, int local_i);                /* doubles in the fab    */
int  vdn_multifab_dataptr(const vdn_multifab *mf, int local_i, double **dev);   /* dataptr (DEVICE ptr)  */
int  vdn_multifab_copy_to_host(const vdn_multifab *mf, int local_i, double *host);
int  vdn_multifab_copy_from_host(vdn_multifab *mf, int local_i, const double *host);
int  vdn_multifab_setval(vdn_multifab *mf, double val, int comp, int nc, int all);     /* setval       */
int  vdn_multifab_copy_c(vdn_multifab *dst, int dcomp, const vdn_multifab *src, int scomp,
                         int nc, int ng);                                               /* copy_c       */
int  vdn_multifab_norm_inf(const vdn_multifab *mf, int comp, int nc, double *out);      /* norm_inf     */
int  vdn_multifab_min_max(const vdn_multifab *mf, int comp, double *mn, double *mx);    /* min_c/max_c  */
int  vdn_multifab_fill_boundary(vdn_multifab *mf);                       /* multifab_fill_boundary    */
int  vdn_multifab_physbc(vdn_multifab *mf, int scomp, int bccomp, int nc,
                         const vdn_bc_tower *bct);                        /* multifab_physbc.f90:17    */

/* ------------------------------------------------------------------------------------------- */
/* the hot path.  Arrays of per-level multifab handles (length nlevel).                         */
/* dx is [nlevel][3].  press_comp is the 1-based bc component (dm+nscal+1) as in the reference. */
/* sold / snew / ext_scal_force carry nscal components, any nscal vdn_init accepted (1..11):   */
/* component 1 (0-based 0) is the density, the others are passive tracers.                    */
/* ------------------------------------------------------------------------------------------- */
int  vdn_advance_timestep(int istep, vdn_layout *mla,
                          vdn_multifab **sold, vdn_multifab **uold,
                          vdn_multifab **snew, vdn_multifab **unew,
                          vdn_multifab **gp,   vdn_multifab **p,
                          vdn_multifab **ext_vel_force, vdn_multifab **ext_scal_force,
                          const vdn_bc_tower *the_bc_tower,
                          double dt, double time, const double *dx,
                          int press_comp, int proj_type);
/* estdt(lev,u,s,gp,ext_vel_force,dx,dtold,dt)  (reference src/estdt.f90:15-87) */
int  vdn_estdt(int lev, const vdn_multifab *u, const vdn_multifab *s, const vdn_multifab *gp,
               const vdn_multifab *ext_vel_force, const double *dx /*[3]*/, double dtold, double *dt);
/* hgproject(proj_type,mla,unew,uold,rhohalf,p,gp,dx,dt,the_bc_tower,press_comp)
 * (reference src/hgproject.f90:17) */
int  vdn_hgproject(int proj_type, vdn_layout *mla, vdn_multifab **unew, vdn_multifab **uold,
                   vdn_multifab **rhohalf, vdn_multifab **p, vdn_multifab **gp,
                   const double *dx, double dt, const vdn_bc_tower *bct, int press_comp);
/* macproject(mla,umac,rho,mac_rhs,dx,the_bc_tower,bc_comp)  (reference src/macproject.f90:20);
 * umac is [nlevel][3] */
int  vdn_macproject(vdn_layout *mla, vdn_multifab **umac, vdn_multifab **rho, vdn_multifab **mac_rhs,
                    const double *dx, const vdn_bc_tower *bct, int bc_comp);

/* ---- multi-level operators (FBoxLib; up to 4 levels, refinement ratio 2, boxes on any rank) ---------------------------------
 * ml_cc_restriction(crse, fine, rr)            reference call sites src/macproject.f90:204-206, src/hgproject.f90:355-357
 * ml_edge_restriction(crse, fine, rr, dir)     src/velpred.f90:115-119, src/macproject.f90:330-333, 497-500
 * multifab_fill_ghost_cells(fine, crse, ...)   src/macproject.f90:304-310 (and inside ml_restrict_and_fill)
 * create_umac_grown(fine, crse, ...)           src/velpred.f90:102-107, src/macproject.f90:107-113
 * ml_restrict_and_fill(nlevs, mf, rr, bc, icomp, bcomp, nc, same_boundary)   src/update.f90:103-107, src/mkforce.f90:75-76, ...
 * components 0-based.  vdn_macproject / vdn_hgproject / vdn_advance_timestep accept nlevel = 2..4 (composite solves); umac is then [lev*3 + dir]. */
int vdn_ml_cc_restriction(vdn_multifab *crse, const vdn_multifab *fine, int icomp, int nc);
int vdn_ml_edge_restriction(vdn_multifab *crse, const vdn_multifab *fine, int dir);
int vdn_multifab_fill_ghost_cells(vdn_multifab *fine, const vdn_multifab *crse, int icomp, int nc);
int vdn_create_umac_grown(vdn_multifab *fine, const vdn_multifab *crse, int dir);
int vdn_ml_restrict_and_fill(int nlev, vdn_multifab **mf, int icomp, int bcomp, int nc, int same_boundary, const vdn_bc_tower *bct);

/* regridding (src/regrid.f90:280-337, build_and_fill_data): fillpatch(fine, crse, ng = 0, ...) fills every valid cell of a new fine
 * level from the coarser one (coarse ghost cells filled; interpolation of multifab_fill_ghost_cells); ml_nodal_prolongation does the
 * same for the nodal pressure (trilinear); multifab_copy_c between multifabs of one level whose box lists differ copies the points
 * valid in both (old data over the interpolated data). */
int vdn_fillpatch(vdn_multifab *fine, const vdn_multifab *crse, int icomp, int nc);
int vdn_ml_nodal_prolongation(vdn_multifab *fine, vdn_multifab *crse);
int vdn_multifab_copy_layouts(vdn_multifab *dst, int dcomp, const vdn_multifab *src, int scomp, int nc);

/* ---- grid generation in front of the AMR path ------------------------------------------------------------------------------------
 * tag_boxes(mf, tagboxes, dx, lev)                               src/tag_boxes.f90:17-48 (rules :142-210: rho > 1.01 / 1.1 / 1.5 by level
 *                                                                for prob_type 1, 2; 1.2 < rho < 1.8 for prob_type 3)
 * make_new_grids(new_grid, la_crse, la_fine, mf, dx, buf_wid, ref_ratio, lev, max_grid_size)   [FBoxLib]   src/initialize.f90:247-248,
 *                                                                src/regrid.f90:148-149; cluster_* parameters src/_parameters:37-39
 * s: the state of level `lev1` (1-based, as in tag_boxes) -- component 0 is tagged; the boxes of level lev1+1 are returned in that
 * level's index space (*nboxes_out = 0: no cell tagged, "new_grid = .false.").  nest: cells of level lev1 kept between the new
 * level and the edge of level lev1 (proper nesting).  Collective: every rank passes its part of the level and gets the same boxes. */
/* tag_boxes(tagboxes, mf, dx, lev) of src/tag_boxes.f90:17-216 alone: one byte per cell of the level's domain (x fastest), 1 = tagged;
 * lev1 is the 1-based level the thresholds are chosen by (tag_boxes.f90:65-94, 142-178) */
int vdn_tag_boxes(const vdn_multifab *s, int lev1, unsigned char *tags_host);
int vdn_make_new_grids(const vdn_multifab *s, int lev1, int buf_wid, int nest, double min_eff, int min_width, int blocking,
                       int max_grid_size, int maxboxes, vdn_box *boxes_out, int *nboxes_out, long *ntagged);

/* ---- refinement criteria chosen at run time ----------------------------------------------------------------------------------------
 * The stand-in for editing src/tag_boxes.f90 (the file a user of the reference rewrites per problem; its aux_tag_mf hook ends in bl_error):
 * a valid cell of level lev1 (1-based) is tagged when, for ANY of the ncrit criteria (1 .. VDN_TAG_MAX_CRITERIA),
 *        gt[lev1-1] < value < lt[lev1-1]            both strict, as in tag_boxes.f90
 * where `value` is what `field` names.  +-HUGE_VAL leaves a side open; gt = +HUGE_VAL switches the criterion off on that level; a NaN value
 * tags nothing.  `comp` (0-based) is the component of s a SCALAR / SCALAR_GRAD criterion reads; velocity criteria ignore it.  All criteria are
 * evaluated per cell in one pass on the device; no vorticity or gradient multifab is built.
 *   VDN_TAG_VORTICITY, VDN_TAG_MAGVEL: the value vdn_make_vorticity / vdn_make_magvel would store for the same u, bit for bit (the same device
 *     arithmetic), dm = 2: |v_x - u_y|.  The call fills the ghost cells of u the way those two do: the same-level fill, then (vorticity) physbc
 *     -- so u is not const.  They need u; the vorticity also dx[dm] and the bc tower, and one ghost cell on u.
 *   VDN_TAG_SCALAR_GRAD reads ONE ghost layer of s and fills nothing: the caller has filled it (same level, physical boundary), as the drivers
 *     do before every regrid.
 *   Ghost cells at a coarse-fine boundary are the caller's in both cases (vdn_ml_restrict_and_fill).
 * u, dx and bct may be NULL when no criterion reads the velocity.  Refused (non-zero, vdn_last_error): an unknown field, a comp outside s, ncrit
 * outside 1 .. 8, a velocity criterion without u, a gradient criterion on a state without ghost cells.
 * vdn_tag_boxes_by / vdn_make_new_grids_by are vdn_tag_boxes / vdn_make_new_grids with this rule in place of the reference's; everything after the
 * tag bitmap (the OR over the ranks, buffer, nesting, clustering, chop) is the same code.  dm = 2 and dm = 3 layouts. */
#ifndef VDN_MAXLEV
#define VDN_MAXLEV 4          /* deepest hierarchy (levels) */
#endif
#define VDN_TAG_SCALAR       0   /* s(comp) */
#define VDN_TAG_SCALAR_GRAD  1   /* max over d < dm of max(|s(i+e_d) - s(i)|, |s(i) - s(i-e_d)|), undivided */
#define VDN_TAG_VORTICITY    2   /* the value vdn_make_vorticity writes (dm = 2: its absolute value) */
#define VDN_TAG_MAGVEL       3   /* the value vdn_make_magvel writes */
#define VDN_TAG_MAX_CRITERIA 8
typedef struct { int field; int comp; double gt[VDN_MAXLEV]; double lt[VDN_MAXLEV]; } vdn_tag_criterion;
int vdn_tag_boxes_by(const vdn_multifab *s, vdn_multifab *u, const double *dx, const vdn_bc_tower *bct, int lev1,
                     int ncrit, const vdn_tag_criterion *crit, unsigned char *tags_host);
int vdn_make_new_grids_by(const vdn_multifab *s, vdn_multifab *u, const double *dx, const vdn_bc_tower *bct, int lev1,
                          int ncrit, const vdn_tag_criterion *crit,
                          int buf_wid, int nest, double min_eff, int min_width, int blocking,
                          int max_grid_size, int maxboxes, vdn_box *boxes_out, int *nboxes_out, long *ntagged);

/* ---- derived plot quantities of write_plotfile (src/varden.f90:532-540) ------------------------------------------------------------
 * make_vorticity(vort, comp, u, dx, bc)   src/makevort.f90:16-57  (fills the ghost cells of u first, as the reference does;
 *                                         3-D: |curl u| with one-sided differences next to inflow / no-slip faces, 2-D: v_x - u_y)
 * make_magvel(magvel, comp, u)            src/makevort.f90:59-91
 * comp 0-based. */
int vdn_make_vorticity(vdn_multifab *vort, int comp, vdn_multifab *u, const double *dx /*[dm]*/, const vdn_bc_tower *bct);
int vdn_make_magvel(vdn_multifab *magvel, int comp, vdn_multifab *u);

/* ---- run diagnostics on the device: integrals, extrema and a finite check over the composite grid ------------------------------------
 * No reference counterpart (multifab_min_c / max_c of src/hgproject.f90:89-95 is the nearest).  Every quantity runs over the COMPOSITE grid -- the valid
 * cells of level n that no box of level n + 1 covers -- and every cell is weighted by its own dx dy dz (dm = 2: dx dy, one z plane).  u[nlev], s[nlev]: the
 * velocity and the scalars of every level on the layout mla; dx: [nlev][3].  Component 0 of s is the density.
 *   counts     cells, cells_lev; nonfinite: composite cells where any component of u or s is NaN or +-Inf (exact)
 *   integrals  volume, volume_lev; sum_s[c] = int s_c dV (c = 0: the mass); momentum[d] = int rho u_d dV; kinetic = 1/2 int rho |u|^2 dV;
 *              enstrophy = 1/2 int w^2 dV, w the value vdn_make_vorticity stores (dm = 3: |curl u|, dm = 2: v_x - u_y)
 *   extrema    exact: the bits of a value that is in the field; -0 sorts below +0 (as in the plot files' Cell_H); magvel as vdn_make_magvel
 * Entries beyond nscal, dm or nlev are 0.  enstrophy, vort_min and vort_max are computed only with VDN_DIAG_VORT in `what` (0 otherwise); they read ONE GHOST
 * LAYER of u and, unlike vdn_make_vorticity, the call FILLS NOTHING: the caller has filled it (same level, physical boundary, coarse-fine: what the drivers do at
 * the top of every step).  Without VDN_DIAG_VORT no ghost cell is read, and bct may be NULL.  The call reads its inputs and writes none of them.
 * Deterministic: sums are added in a fixed order (inside a slab of a box, then slab by slab in level / box / k order), never by atomics -- two calls give the
 * same bits, every rank gets the same bits, and the bits do not depend on the number of ranks (they do depend on how a level is cut into boxes).  Collective.
 * Refused (non-zero, vdn_last_error): nlev outside 1 .. 4 or not the layout's; u / s not on mla (or on different box lists); a NULL dx; a NULL bct or u without
 * a ghost cell with VDN_DIAG_VORT; dm = 2 with nlev > 1. */
#define VDN_DIAG_VORT 1
typedef struct vdn_diag {
  long long cells, cells_lev[4], nonfinite;
  double volume, volume_lev[4];
  double sum_s[11], momentum[3], kinetic, enstrophy;
  double s_min[11], s_max[11], u_min[3], u_max[3], magvel_max, vort_min, vort_max;
} vdn_diag;
int vdn_diagnostics(int nlev, vdn_layout *mla, vdn_multifab *const *u, vdn_multifab *const *s,
                    const double *dx /*[nlev][3]*/, const vdn_bc_tower *bct, int what, vdn_diag *out);
size_t vdn_diag_sizeof(void);

/* ---- plane-averaged profiles of a hierarchy along one axis, computed on the device -------------------------------------------------------
 * No reference counterpart.  nlev levels, axis a (0 .. dm-1), L = nlev - 1 the finest level OF THE HIERARCHY, whether or not it covers a given plane.
 *   bins      the planes of level L's index space along a: nbins = ncells_a(level 0) << L; bin m is m h <= x_a < (m + 1) h, h = dx[L][a]
 *   cells     the composite grid exactly as vdn_diagnostics defines it: the valid cells of level l that no box of level l + 1 covers.  Such a cell with index i_a
 *             along a lies in the r = 1 << (L - l) bins i_a r .. i_a r + r - 1 and contributes to EACH of them with the weight w_l = (dx dy dz of level l) / r
 *             (dm = 2: dx dy / r); w_l is formed once per level on the host (the division by a power of two is exact)
 *   rows      per bin, rho = s_0; products are associated as written, left to right, then multiplied by w_l:
 *               volume      (number of the bin's composite cells of level l) * w_l, added over the levels       1
 *               s[c]        s_c w_l                                                                          nscal
 *               ss[c]       (s_c s_c) w_l                                                                    nscal
 *               u[d]        u_d w_l                                                                          dm
 *               ru[d]       (rho u_d) w_l                                                                    dm
 *               ruu[d,e]    ((rho u_d) u_e) w_l, d <= e, in the order (0,0) (0,1) [(0,2)] (1,1) [(1,2) (2,2)]    dm (dm + 1) / 2
 *               sua[c]      (s_c u_a) w_l, c >= 1: the flux of tracer c along the axis                        nscal - 1
 *               s_min[c], s_max[c], u_min[d], u_max[d]   exact extrema over the bin's composite cells (the bits of a value that is in the field; -0 sorts
 *                           below +0, as in vdn_diagnostics); 0 where a bin holds no cell                     2 nscal + 2 dm
 *             and, in an array of its own, cells[m]: the number of composite cells lying in bin m (a coarse cell counts in each of its r bins).
 * A plane average is row / volume; the host wrappers offer it, the library does not.  vdn_profiles_layout fills the offsets of the row groups and their count nrow
 * for (dm, nscal) -- a pure host function, callable before vdn_init; a caller never hard-codes a row number.  The result is out[nrow][nbins], row-major, and
 * cells[nbins].  u[nlev], s[nlev]: the velocity and the scalars of every level on the layout mla; dx: [nlev][3].
 * No ghost cell is read, the call writes none of its inputs.  Collective; every rank receives the full result.  Deterministic: sums are added in a fixed order
 * (inside a piece of a box, then slot by slot in level / box / piece order), never by atomics -- two calls give the same bits, every rank gets the same bits, and
 * the bits do not depend on the number of ranks (they do depend on how a level is cut into boxes).
 * vdn_profiles_nbins returns the number of bins, or -1 (vdn_last_error) for a NULL layout, an nlev that is not the layout's or an axis outside 0 .. dm-1.
 * vdn_profiles refuses (non-zero, vdn_last_error, nothing left allocated): an uninitialised library; nlev outside 1 .. 4 or not the layout's; u / s not on mla
 * (or on different box lists); a NULL dx, out or cells; axis outside 0 .. dm-1; nbins other than vdn_profiles_nbins; dm = 2 with nlev > 1. */
typedef struct vdn_profile_layout { int nrow, volume, s, ss, u, ru, ruu, sua, s_min, s_max, u_min, u_max; } vdn_profile_layout;
int  vdn_profiles_layout(int dm, int nscal, vdn_profile_layout *lay);
size_t vdn_profile_layout_sizeof(void);
long vdn_profiles_nbins(int nlev, vdn_layout *mla, int axis);
int  vdn_profiles(int nlev, vdn_layout *mla, vdn_multifab *const *u, vdn_multifab *const *s, const double *dx /*[nlev][3]*/,
                  int axis, long nbins, double *out_host /*[nrow][nbins]*/, long long *cells_host /*[nbins]*/);

/* ---- how much of the fluid has which value: PDFs and conditional sums of a hierarchy's fields, computed on the device (csrc/pdf.hip) -------
 * No reference counterpart.  vdn_profiles bins by position; these two bin by VALUE.
 *   cells     the composite grid exactly as vdn_diagnostics defines it: the valid cells of level l that no box of level l + 1 covers.  A cell of level l carries
 *             dV_l = dx dy dz of its level (dm = 2: dx dy).
 *   bin field q, chosen by (field, comp), comp 0-based:
 *               VDN_PDF_SCALAR     s(comp), comp 0 .. nscal-1
 *               VDN_PDF_VELOCITY   u(comp), comp 0 .. dm-1
 *               VDN_PDF_MAGVEL     the velocity magnitude, bit for bit the value vdn_make_magvel stores for the same u (comp is not read)
 *               VDN_PDF_VORTICITY  the vorticity, bit for bit the value vdn_make_vorticity stores for the same u (comp is not read): its magnitude for dm = 3, signed
 *                                  for dm = 2.  It reads ONE ghost layer of u, which the caller has filled, and needs bct, as VDN_DIAG_VORT does.
 *             The other three fields read no ghost cell.
 *   slots     the axis is {field, comp, nbins, lo, hi} with w = (hi - lo) / nbins formed once on the host in double.  nbins + 2 slots: slot 0 is "below", slots
 *             1 .. nbins are the bins, slot nbins + 1 is "above".  In this order (csrc/pdf_bin.h):
 *               1.  q != q: the cell counts in nan_cells and in nothing else
 *               2.  q <  lo: slot 0
 *               3.  q >= hi: slot nbins + 1
 *               4.  otherwise m = (int)floor((q - lo) / w), a true division, not contracted; m is clamped to nbins - 1; the slot is 1 + m
 *             +-Inf fall out of rules 2 and 3; -0 with lo = 0 lands in bin 0.
 * vdn_pdf, one axis, nbins 1 .. VDN_PDF_MAX_BINS, returns
 *   cells[VDN_MAXLEV][nbins + 2]   the exact number of composite cells of each level in each slot (0 beyond nlev)
 *   nan_cells                      the composite cells whose q is NaN
 *   out[nrow][nbins + 2]           row-major; rho = s_0; products are associated as written and then multiplied by dV_l:
 *               volume      not summed per cell: the sum over the levels 0 .. nlev-1, ascending, of cells[l][slot] * dV_l        1
 *               q           q dV_l                                                                                               1
 *               s[c]        s_c dV_l                                                                                             nscal
 *               u[d]        u_d dV_l                                                                                             dm
 *               ru[d]       (rho u_d) dV_l                                                                                       dm
 *               ke          ((0.5 rho) (u.u)) dV_l, u.u added as the velocity magnitude adds it: (u_0 u_0 + u_1 u_1) [+ u_2 u_2]     1
 * vdn_pdf_layout fills the first row of every group and nrow = nscal + 2 dm + 3 for (dm, nscal) -- a pure host function, callable before vdn_init; a caller never
 * hard-codes a row number.  The PDF itself is volume[1 .. nbins] / (sum of volume * w), a conditional mean is row / volume: the host wrappers offer both, the library
 * does not.  A NaN (or Inf - Inf) in a summed field of a cell whose q is finite makes that slot's row NaN; the counts and volume stay exact.
 * vdn_pdf2, two axes, each nbins 1 .. VDN_PDF2_MAX_BINS, returns cells[VDN_MAXLEV][n1 + 2][n2 + 2], volume[n1 + 2][n2 + 2] formed from the counts as above, and
 * nan_cells, which counts a cell when EITHER value is NaN.  Counts only, no conditional sums.
 * Both calls write none of their inputs and are collective; every rank receives the full result.  Deterministic: counts are integers; sums are added in a fixed order
 * (inside a slab of a box by a fixed thread map and tree, then slab by slab in level / box / k order), never by floating-point atomics -- two calls give the same bits,
 * every rank gets the same bits, and the bits do not depend on the number of ranks (they do depend on how a level is cut into boxes).  Every temporary lives in the
 * arena for the duration of the call.
 * Both refuse (non-zero, vdn_last_error, nothing left allocated, a following call unaffected): an uninitialised library; NULL arguments (mla, u, s, dx, an output);
 * nlev outside 1 .. 4 or not the layout's; u / s not on mla or on different box lists; a field code outside 0 .. 3; comp out of range for VDN_PDF_SCALAR /
 * VDN_PDF_VELOCITY; nbins out of range; a non-finite lo or hi, or !(lo < hi); VDN_PDF_VORTICITY with a NULL bct or a u without a ghost layer; dm = 2 with nlev > 1;
 * a refinement ratio other than 2. */
enum { VDN_PDF_SCALAR = 0, VDN_PDF_VELOCITY = 1, VDN_PDF_MAGVEL = 2, VDN_PDF_VORTICITY = 3 };
#define VDN_PDF_MAX_BINS 256
#define VDN_PDF2_MAX_BINS 64
typedef struct vdn_pdf_layout_t { int nrow, volume, q, s, u, ru, ke; } vdn_pdf_layout_t;    /* (the entry below has the plain name) */
int  vdn_pdf_layout(int dm, int nscal, vdn_pdf_layout_t *lay);
size_t vdn_pdf_layout_sizeof(void);
int  vdn_pdf(int nlev, vdn_layout *mla, vdn_multifab *const *u, vdn_multifab *const *s, const double *dx /*[nlev][3]*/, const vdn_bc_tower *bct,
             int field, int comp, int nbins, double lo, double hi,
             double *out_host /*[nrow][nbins+2]*/, long long *cells_host /*[VDN_MAXLEV][nbins+2]*/, long long *nan_cells);
int  vdn_pdf2(int nlev, vdn_layout *mla, vdn_multifab *const *u, vdn_multifab *const *s, const double *dx /*[nlev][3]*/, const vdn_bc_tower *bct,
              int field1, int comp1, int nbins1, double lo1, double hi1, int field2, int comp2, int nbins2, double lo2, double hi2,
              long long *cells_host /*[VDN_MAXLEV][n1+2][n2+2]*/, double *volume_host /*[n1+2][n2+2]*/, long long *nan_cells);

/* ---- where a field takes a value: the isosurface q = iso of a hierarchy's field, extracted on the device (csrc/iso.hip, csrc/iso_cell.h) ------
 * No reference counterpart; dm = 3 only.  The library is built -ffp-contract=off, so every expression below has the order written.
 *   cells     the composite grid exactly as vdn_diagnostics defines it: the valid cells of level l that no box of level l + 1 covers.  Each such cell is cut on its own;
 *             the pieces tile the domain without gap or overlap.
 *   field     mf[nlev], comp, bccomp as vdn_sample_points takes them: any cell-centred multifab with at least one ghost layer, which the CALLER has filled (same level,
 *             physical boundary, coarse-fine).  The call fills nothing and writes none of its inputs.
 *   nodes     node (i, j, k) of level l is the low corner of cell (i, j, k), at (i dx, j dy, k dz): one multiplication per direction.  Its value comes from the eight
 *             cells (i-1..i, j-1..j, k-1..k), read from the fab of the box that owns the cell being cut, as a pairwise mean m = 0.5 a + 0.5 b along x, then along y,
 *             then along z.  The face-value rule of vdn_sample_points: where the node lies on a domain face whose adv boundary type of component bccomp is EXT_DIR, the
 *             ghost cell holds the value ON the face; along that direction m is the ghost value alone.  A cell forms its eight nodes itself; the same expression on the
 *             same values gives the same bits in every cell of a level that shares the node (a same-level ghost cell holds its neighbour's bits).
 *   tetrahedra   six Kuhn tetrahedra around the diagonal (0,0,0)-(1,1,1): for the axis orders (x,y,z), (x,z,y), (y,x,z), (y,z,x), (z,x,y), (z,y,x), in this order,
 *             v0 = corner (0,0,0), v1 = v0 + e_a, v2 = v1 + e_b, v3 = (1,1,1).  The triangulation matches across the faces of neighbouring cells of a level: the
 *             surface is watertight within a level.
 *   above     a vertex is above when q > iso (strict).  An edge is crossed between a not-above end A and an above end B, so q_B - q_A > 0 always:
 *             t = (iso - q_A) / (q_B - q_A), p_d = x_A,d + t (x_B,d - x_A,d), always from A to B: two tetrahedra that share the edge form the same bits.
 *   triangles one or three vertices above: one triangle; two: two; none or four: none.  (p1 - p0) x (p2 - p0) points towards the not-above side.  csrc/iso_cell.h holds the
 *             case table, once, and states the vertex order of every case.
 *   sums      per triangle the area 0.5 |cross|, cross = (p1 - p0) x (p2 - p0), |c| = sqrt((c_x c_x + c_y c_y) + c_z c_z), and area_vec 0.5 cross (a closed surface sums
 *             to zero).  The volume above under the linear interpolant, V_tet = ((dx dy) dz) / 6: one vertex above ((V_tet (1 - t1)) (1 - t2)) (1 - t3); three above
 *             V_tet - ((V_tet t1) t2) t3; four V_tet; two: the wedge as three tetrahedra, each |det| / 6 -- csrc/iso_cell.h writes the association.  A cell's sums start
 *             from +0 and take tetrahedron 0 .. 5, triangle 0 .. 1 in order.
 *   non-finite   a cell with a non-finite node value emits nothing, adds nothing and is counted in nonfinite_cells.
 *   order     level, then global box number, then cell with i fastest, then j, then k; inside a cell tetrahedron 0 .. 5, then triangle 0 .. 1: a function of the box lists
 *             and the field alone.
 *   levels    the two sides of a coarse-fine face see different node values: the surface has cracks there.  Area and volume still tile, because the cells do.
 * vdn_iso: ntri, cut_cells (the cells that emit a triangle), their parts per level, nonfinite_cells; area and its parts per level, area_vec, volume_above; volume: the
 * volume of the cells that were cut up -- all composite cells but the non-finite ones --, the sum over the levels, ascending, of their number times dx dy dz of the level.
 * The counts and sums are always returned.  Triangles ([ntri][vertex][direction]) and their levels are written only when tri_host is given and ntri <= max_tri; written
 * is then ntri, else 0 and the buffers are untouched: a caller sizes a second call from the first.  lev_host may be NULL.
 * Collective; every rank receives the full result.  Deterministic: counts are integers, sums run in a fixed order (thread map, trees, then slab by slab in output order),
 * positions come from integer scans, no atomic takes part: two calls give the same bits and the bits do not depend on the number of ranks.  Every temporary lives in the
 * arena for the duration of the call.
 * Refuses (non-zero, vdn_last_error, nothing left allocated, a following call unaffected): what vdn_sample_points refuses -- an uninitialised library; NULL mla, mf, dx,
 * bct, out; nlev outside 1 .. 4 or not the layout's; a bc tower of another layout; a dx that is not positive and finite; a level's mf NULL, of another layout or level,
 * nodal, without component comp or without a ghost layer; bccomp outside the tower --, and: a non-finite iso; dm = 2; a refinement ratio other than 2; max_tri < 0;
 * max_tri > 0 with a NULL tri_host.
 * vdn_isosurface_write: binary PLY, little endian -- "ply", "format binary_little_endian 1.0", "comment VDN_ISO 1 iso <%.17g> time <%.17g>", "element vertex <3 ntri>" with
 * "property double x / y / z", "element face <ntri>" with "property list uchar int vertex_indices" and "property uchar level", "end_header"; then the vertices and the
 * faces (3, three indices, the level): a triangle soup, no vertex merged.  Rank 0 writes; the same arguments give the same bytes.  A host function: it needs no
 * vdn_init.  Refuses a NULL path, ntri < 0 or 3 ntri beyond 32 bits, triangles without tri_host and lev_host, a file it cannot write. */
typedef struct vdn_iso {
  long long ntri, ntri_lev[4], cut_cells, cut_cells_lev[4], nonfinite_cells, written;
  double area, area_lev[4], area_vec[3], volume_above, volume;
} vdn_iso;
size_t vdn_iso_sizeof(void);
int  vdn_isosurface(int nlev, vdn_layout *mla, vdn_multifab *const *mf, int comp, int bccomp, const double *dx /*[nlev][3]*/, const vdn_bc_tower *bct, double iso,
                    long long max_tri, double *tri_host /*[max_tri][3][3] or NULL*/, unsigned char *lev_host /*[max_tri] or NULL*/, vdn_iso *out);
int  vdn_isosurface_write(const char *path, long long ntri, const double *tri_host, const unsigned char *lev_host, double iso, double time);
/* vdn_isosurface with the form of its second pass chosen by the caller -- 0: every cell forms its nodes and counts again, 1: the first pass stores a count per cell and the
 * second reads it, loading the neighbourhood of cut cells alone -- and ms[0], ms[1]: the device time in milliseconds of the launches of pass 1 and pass 2 (events
 * around them; 0 for a pass that did not run).  The same refusals, and a form other than 0 or 1 or a NULL ms; the same bits from both forms.  It exists for the
 * measurement that chose the form vdn_isosurface runs (tools/iso_probe.py). */
int  vdn_isosurface_timed(int nlev, vdn_layout *mla, vdn_multifab *const *mf, int comp, int bccomp, const double *dx /*[nlev][3]*/, const vdn_bc_tower *bct, double iso,
                          long long max_tri, double *tri_host, unsigned char *lev_host, vdn_iso *out, int form, double *ms /*[2]*/);

/* ---- values at points and Lagrangian tracer particles (csrc/particles.hip, csrc/particle_plan.h).  No reference counterpart -------------
 * Positions are physical, measured from the domain's low corner (prob_lo = 0); level l has spacing dx[l][d]; dm = 2 uses x and y (z is stored as 0).  The
 * domain's extent is len_d = ncells_d(level 0) * dx[0][d]; a point is inside when 0 <= x_d <= len_d in every direction.
 * Host cell and level: on level l the cell of a point is c_d = floor(x_d / dx[l][d]) (a true division), clamped to the level's domain, so that a point on the
 * high domain face belongs to the last cell.  The host level is the FINEST level with a box whose valid region holds that cell (one lookup per level in a map
 * over blocks, csrc/particle_plan.h; never a loop over boxes).
 * Interpolation, trilinear (bilinear in dm = 2): xi_d = x_d / dx_d - 0.5, i_d = floor(xi_d), w_d = xi_d - i_d; the eight cells i_d, i_d + 1 are read from the
 * HOST BOX's own fab -- at most one ghost layer, which the CALLER has filled (the call fills nothing) --; seven lerps a + w (b - a), along x, then y, then z.
 * Face values: where the adv boundary type of component bccomp + c at a domain face is VDN_EXT_DIR the ghost cell holds the value ON the face (multifab_physbc's
 * convention); in the half cell next to such a face the weight along that direction is 2 xi_d + 1 (low face, i_d = lo - 1) or 2 w_d (high face, i_d = hi), for
 * that component alone.  Every other ghost value counts as cell-centred.
 * Move (Heun between two time levels): k1 = u0(x); x* = bc(x + dt k1); k2 = u1(x*); x' = bc(x + (0.5 dt)(k1 + k2)).  bc, per direction: periodic -- p + len
 * below 0, p - len from len on; SLIP_WALL, NO_SLIP_WALL, SYMMETRY -- -p below 0, len - (p - len) above len; then (both) clamped to [0, len]; INLET, OUTLET --
 * crossed by x*: k2 := k1; crossed by x': the particle keeps its position, gets state 1 ("left") and is never sampled (value 0, level -1) or moved again.
 * Particles keep their index.  Several ranks: every rank holds all particles, evaluates those whose host box it owns, writes +0.0 for the rest, and one sum
 * all-reduce per stage fills them in (x + 0 + ... + 0 = x): the same bits on any number of ranks.  The calls are collective.
 * Every call refuses (non-zero, vdn_last_error, nothing left allocated): an uninitialised library, null arguments, nlev other than the layout's, multifabs not
 * on mla / nodal / with fewer than comp + nc components / without a ghost layer, a null bct or dx, n < 1, dm = 2 with nlev > 1, a level whose block map would
 * exceed 2^25 entries (level and block size named), a face type without a rule. */
typedef struct vdn_particles vdn_particles;
/* mf's components comp .. comp + nc - 1 (nc <= 16) at n points: val_host[n][nc], lev_host[n] (may be NULL) = the host level; a point outside the domain (or not
 * finite) gets level -1 and value 0 */
int vdn_sample_points(int nlev, vdn_layout *mla, vdn_multifab *const *mf, int comp, int nc, int bccomp, const double *dx /*[nlev][3]*/,
                      const vdn_bc_tower *bct, long n, const double *x_host /*[n][3]*/, double *val_host /*[n][nc]*/, int *lev_host /*[n]*/);
/* n particles at x_host[n][3], state 0.  Refuses a non-finite position here; a position outside the domain at the first call that names the hierarchy */
int vdn_particles_create(long n, const double *x_host /*[n][3]*/, vdn_particles **P);
int vdn_particles_destroy(vdn_particles *P);
/* n: the particles; active: those with state 0 (either may be NULL) */
int vdn_particles_count(vdn_particles *P, long *n, long *active);
/* positions x_host[n][3] and states state_host[n] (either may be NULL) */
int vdn_particles_get(vdn_particles *P, double *x_host, int *state_host);
/* one move; u0, u1: the velocity (components 0 .. dm-1, boundary components 0 .. dm-1) at the old and the new time, ghost cells filled */
int vdn_particles_advance(vdn_particles *P, int nlev, vdn_layout *mla, vdn_multifab *const *u0, vdn_multifab *const *u1,
                          const double *dx /*[nlev][3]*/, const vdn_bc_tower *bct, double dt);
/* vdn_sample_points at the particles' positions, which stay on the device; a particle that left gets value 0 and level -1 */
int vdn_particles_sample(vdn_particles *P, int nlev, vdn_layout *mla, vdn_multifab *const *mf, int comp, int nc, int bccomp,
                         const double *dx /*[nlev][3]*/, const vdn_bc_tower *bct, double *val_host /*[n][nc]*/, int *lev_host /*[n], may be NULL*/);
/* one file (rank 0 writes): the text lines "VDN_PARTICLES 1", "dm D", "n N", "ncol C", the C names (one word each), "time T" (17 significant digits), then
 * little-endian int32 state[n], float64 x[n][3], float64 cols[ncol][n].  read: positions and states (the columns are the caller's to parse); a read followed
 * by a write of the same columns gives the same bytes.  read refuses a file that is short, has another first line, or another dm than the run */
int vdn_particles_write(vdn_particles *P, const char *path, double time, int ncol, const char *const *names, const double *cols /*[ncol][n]*/);
int vdn_particles_read(const char *path, vdn_particles **P, double *time);

/* ---- plot files and checkpoints (FBoxLib's fabio_module and the reference's checkpoint_module) ------------------------------------------------------
 * The files are the ones varden_amd/plotfile.py defines (Header, Level_NN/Cell_H with es27.17e3 numbers, Level_NN/Cell_D_00000 with a FAB line in front of
 * every fab's doubles), byte for byte.  The valid points of every fab are packed on the device into a staging buffer of `staging_bytes` (<= 0: 256 MB; neither
 * the device nor the pinned host buffer is made larger than the largest level), copied to the host and written, range by range; Cell_H's per-fab minima and
 * maxima are exact and come out of the same pass (-0 sorts below +0).  ONE RANK: with nranks > 1 the writers and the reader fail ("several ranks: use the
 * Python writer").  Every failed fopen / fwrite / short read / foreign FAB line fails the call with the path and strerror in vdn_last_error().
 * vdn_fabio_ml_multifab_info, _boxes and vdn_checkpoint_info only parse text: they need neither vdn_init nor a GPU. */
/* fabio_ml_multifab_write_d as src/varden.f90:568-573 and src/checkpoint.f90:45-48 call it: mfs[nlev] share components and nodal flags; rr[nlev-1] */
int vdn_fabio_ml_multifab_write_d(const char *dirname, int nlev, vdn_multifab *const *mfs, const int *rr,
        const char *const *names, const vdn_box *pd0, const double *prob_lo, const double *prob_hi,
        double time, const double *dx0, long staging_bytes);   /* NULL names, pd0, prob_lo, prob_hi, dx0: the defaults plotfile.write_ml_multifab takes */
/* what fabio_ml_multifab_read_d (src/checkpoint.f90:116-122) learns from the files before it builds its layout: levels, dimension, components, nodal flags,
 * boxes per level (nboxes[nlev], at most 4), ratios (rr[nlev-1]), time.  Any output pointer may be NULL */
int vdn_fabio_ml_multifab_info (const char *dirname, int *nlev, int *dm, int *ncomp, int nodal[3], int *nboxes, int *rr, double *time);
/* the CELL boxes of one level, in the file's order (the boxarray fabio_ml_multifab_read_d builds its layout from) */
int vdn_fabio_ml_multifab_boxes(const char *dirname, int lev, vdn_box *boxes, int maxboxes);
/* the data part of fabio_ml_multifab_read_d (src/checkpoint.f90:116-122): mfs[lev] is built on the file's box list, in the file's order, with the file's nodal
 * flags and at least its components; valid points are overwritten, ghost cells are not touched.  A mismatch fails naming the level and the box */
int vdn_fabio_ml_multifab_read_d(const char *dirname, int nlev, vdn_multifab *const *mfs, long staging_bytes);
/* checkpoint_write / checkpoint_read, src/checkpoint.f90:14-145: State, Pressure, Header (&CHKPOINT time, dt, nlevs; then the ratios) */
int vdn_checkpoint_write(const char *dirname, int nlev, vdn_multifab *const *state, vdn_multifab *const *pressure,
        const int *rr, double time, double dt, long staging_bytes);
/* the namelist read of checkpoint_read (src/checkpoint.f90:100-112); State and Pressure are then read with vdn_fabio_ml_multifab_info / _boxes / _read_d */
int vdn_checkpoint_info (const char *dirname, int *nlev, double *time, double *dt, int *rr);
/* ---- the same files for a 2-D problem that runs as its z-uniform 3-D copy (vdn_set_extruded_2d): dm = 2 files of plane k = 0 ----------
 * write_plane_d: the arguments of vdn_fabio_ml_multifab_write_d, then comps[ncomp] = the source component of every file component (any order, need not be
 * contiguous; names[ncomp]); pd0, prob_lo, prob_hi, dx0 give their two in-plane entries.  The file boxes of a level are the (x, y) footprints of the boxes
 * that contain plane k = 0 (the node plane k = 0 of a multifab nodal in z), in the multifab's box order; those footprints must be pairwise disjoint and every
 * other box of the level must have exactly one of them, else the call fails naming the level and the box before anything is launched.  The files are what
 * plotfile.write_ml_multifab(dm = 2) writes for the plane arrays, byte for byte.
 * defect (NULL: not asked for) receives two figures over everything written: [0] the largest |f(i,j,k) - f(i,j,0)| over the listed components of all boxes,
 * measured against the plane that goes to the file; [1] the largest |value| over the components vanish[nvanish] (w, gpz), all boxes.  Reported, never judged.
 * read_plane_d: a dm = 2 file into 3-D multifabs cut along z in any way: every box's footprint must equal exactly one file box (else: level and box named),
 * the file's nodal flags are the multifab's in-plane ones, the file holds ncomp components; component c of the file goes to EVERY valid z-plane of comps[c]
 * (nz, or nz + 1 when nodal in z).  Ghost cells and unlisted components are not touched. */
int vdn_fabio_ml_multifab_write_plane_d(const char *dirname, int nlev, vdn_multifab *const *mfs, const int *rr,
        const char *const *names, const vdn_box *pd0, const double *prob_lo, const double *prob_hi,
        double time, const double *dx0, long staging_bytes, int ncomp, const int *comps, int nvanish, const int *vanish, double *defect /*[2]*/);
int vdn_fabio_ml_multifab_read_plane_d(const char *dirname, int nlev, vdn_multifab *const *mfs, long staging_bytes, int ncomp, const int *comps);
/* vdn_checkpoint_write through the plane writer: State = comps[ncomp] of state, Pressure = component 0 of pressure (nodal (1,1) in the file), the same Header.
 * defect: [0] over State and Pressure, [1] over vanish[nvanish] of state */
int vdn_checkpoint_write_plane(const char *dirname, int nlev, vdn_multifab *const *state, vdn_multifab *const *pressure,
        const int *rr, double time, double dt, long staging_bytes, int ncomp, const int *comps, int nvanish, const int *vanish, double *defect /*[2]*/);
/* makevort_2d's rule (src/makevort.f90:93-156: the signed v_x - u_y, one-sided forms over dx next to inflow, slip and no-slip faces) on every plane of a
 * 3-D copy; the ghost fill of u is vdn_make_vorticity's.  dx: the two in-plane spacings */
int vdn_make_vorticity_plane(vdn_multifab *vort, int comp, vdn_multifab *u, const double *dx /*[2]*/, const vdn_bc_tower *bct);

/* per-phase wall seconds of the last vdn_advance_timestep (reference prints them,
 * advance_timestep.f90:159-166): [0]=scalar [1]=velocity [2]=MAC [3]=HG [4]=total              */
int  vdn_last_step_timing(double *sec5);
/* diagnostics of the last MAC / HG solves: cycles, initial and final residual norms             */
int  vdn_last_solver_stats(int which /*0=MAC,1=HG*/, int *cycles, double *res0, double *res);
/* Krylov bottom solvers (vdn_params.mg_bottom_solver / hg_bottom_solver = 1, 2, 3) of the last cell-centred (which = 0) / nodal (which = 1) solve: visits of
 * the bottom level, iterations in all, the most in one visit, breakdowns.  All zero with the bottom sweeps.  A composite solve counts all its cycles on level 0.
 * Reads four numbers back from the device (drains the launch stream); any pointer may be NULL. */
int  vdn_last_bottom_stats(int which /*0=cell-centred,1=nodal*/, int *calls, int *iters, int *max_iters, int *breakdowns);
/* what the last cell-centred (which = 0) / nodal (which = 1) solve ran at its bottom level: 0 the bottom sweeps, 1 a Krylov solver in one workgroup
 * (csrc/krylov_wg.h), 2 the same solver over the whole GPU (csrc/krylov_grid.h: bottom levels of 4913 points and more).  -1: which is neither 0 nor 1.
 * vdn_last_bottom_stats counts either form.  No reference counterpart. */
int  vdn_last_bottom_form(int which /*0=cell-centred,1=nodal*/);
/* how the last macproject solve on one box kept its finest level: 0 interleaved (the level array), 1 by colour (passes and residual on the
 * split arrays).  No reference counterpart: the tests use it to know which kernels they exercised. */
int  vdn_last_mac_level_form(void);

/* ------------------------------------------------------------------------------------------- */
/* unit-test hooks: one per reference kernel, single-level, all local boxes.                    */
/* ------------------------------------------------------------------------------------------- */
/* slope_module (src/slope.f90): slopes of comps [0,nc) in direction dir on [lo-1,hi+1]^3;
 * slope multifab must have ng=1, nc comps; bccomp = 0-based first adv_bc component             */
int  vdn_k_slope(const vdn_multifab *s, vdn_multifab *slope, int dir, int bccomp, const vdn_bc_tower *bct);
/* the slope launch of velpred and mkflux by itself: the slopes of the 2 or 3 components of s (ng >= 3) along x, y and z into sl0, sl1, sl2 (ng = 1, the
 * components of s), on [lo-1,hi+1]^3 of every local box, in the launch form the predictors take; vmax (may be NULL): max |s| over the valid cells */
int  vdn_k_slopes_march(const vdn_multifab *s, vdn_multifab *sl0, vdn_multifab *sl1, vdn_multifab *sl2, int bccomp, const vdn_bc_tower *bct, double *vmax);
/* velpred (src/velpred.f90:16): u(3,ng3), force(3,ng1) -> umac[3] (face, ng1), incl. fill_boundary */
int  vdn_k_velpred(const vdn_multifab *u, vdn_multifab **umac, const vdn_multifab *force,
                   const double *dx, double dt, const vdn_bc_tower *bct);
/* mkflux (src/mkflux.f90:16) */
int  vdn_k_mkflux(const vdn_multifab *s, vdn_multifab **sedge, vdn_multifab **flux,
                  vdn_multifab **umac, const vdn_multifab *force, const vdn_multifab *mac_rhs,
                  const double *dx, double dt, const vdn_bc_tower *bct, int is_vel, const int *is_cons);
/* update (src/update.f90:16), incl. the ghost fill of snew */
int  vdn_k_update(const vdn_multifab *sold, vdn_multifab **umac, vdn_multifab **sedge, vdn_multifab **flux,
                  const vdn_multifab *force, vdn_multifab *snew, const double *dx, double dt,
                  int is_vel, const int *is_cons, const vdn_bc_tower *bct);
/* mkvelforce / mkscalforce (src/mkforce.f90:18,238), incl. ghost fill */
int  vdn_k_mkvelforce(vdn_multifab *vel_force, const vdn_multifab *ext_vel_force, const vdn_multifab *s,
                      const vdn_multifab *gp, const vdn_multifab *lapu /*may be NULL*/, double visc_fac,
                      const vdn_bc_tower *bct);
int  vdn_k_mkscalforce(vdn_multifab *scal_force, const vdn_multifab *ext_scal_force,
                       const vdn_multifab *laps /*may be NULL*/, double diff_fac, const vdn_bc_tower *bct);
/* make_at_halftime (src/make_at_halftime.f90:18) */
int  vdn_k_make_at_halftime(vdn_multifab *rhohalf, const vdn_multifab *sold, const vdn_multifab *snew,
                            int in_comp, int out_comp, const vdn_bc_tower *bct);

/* cell-centred multigrid: solves (-div beta grad) phi = rh with the boundary types
 * bc[dir][side] in {VDN_BC_NEU, VDN_BC_DIR, VDN_BC_PER}; replaces ml_cc_solve as called from
 * reference src/mac_multigrid.f90:53-62 (alpha = 0).  phi has ng=1, rh ng=0, beta[3] faces.      */
int  vdn_cc_solve(vdn_multifab *rh, vdn_multifab *phi, vdn_multifab **beta, const double *dx,
                  const int *bc /*[3][2]*/, double rel_eps, double abs_eps, int max_iter,
                  int *cycles, double *res0, double *res);
/* the same with the alpha term: (alpha - div beta grad) phi = rh, alpha a cell multifab (ng = 0) -- the solve of visc_solve and
 * diff_scalar_solve (src/viscsolve.f90), which mac_multigrid routes through ml_cc_solve too; max_iter >= 0                        */
int  vdn_cc_solve_alpha(vdn_multifab *rh, vdn_multifab *phi, const vdn_multifab *alpha, vdn_multifab **beta, const double *dx,
                        const int *bc /*[3][2]*/, double rel_eps, double abs_eps, int max_iter,
                        int *cycles, double *res0, double *res);
/* one red-black Gauss-Seidel sweep pair (nsweeps times) of that operator on the finest level --
 * the kernel the smoother roofline is quoted on                                                   */
int  vdn_cc_smooth(vdn_multifab *rh, vdn_multifab *phi, vdn_multifab **beta, const double *dx,
                   const int *bc /*[3][2]*/, int nsweeps);
/* nodal multigrid: solves div(sigma grad phi) = div(u) (+rh in) with sigma = coeffs (cell, ng=1,
 * zero outside the domain), dense (Q1) stencil; replaces ml_nd_solve as called from reference
 * src/hg_multigrid.f90:95-105 (add_divu=.true., u=unew).  phi, rh nodal ng=1.                     */
int  vdn_nd_solve(vdn_multifab *rh, vdn_multifab *phi, const vdn_multifab *coeffs, const vdn_multifab *u,
                  const double *dx, const int *bc /*[3][2]*/, double rel_eps, double abs_eps, int max_iter,
                  int *cycles, double *res0, double *res);

/* ---- kernel timing (HIP events on the launch stream) for bench.py's roofline object ---------- */
/* times `nlaunch` back-to-back launches of ONE colour pass of the cc smoother on the finest level
 * and returns the average milliseconds per launch and the number of cells one launch covers.
 * rho (may be NULL): the density behind beta = 2/(rho_i + rho_i-1); given, the pass is the one macproject runs (face coefficients
 * recomputed from rho), otherwise the stored-coefficient pass of the viscous solves and the coarser levels       */
int  vdn_bench_cc_smoother(vdn_multifab *rh, vdn_multifab *phi, vdn_multifab **beta, const vdn_multifab *rho, const double *dx,
                           const int *bc, int nlaunch, double *avg_ms, long *cells);
/* the same passes launched as they are INSIDE a solve: `nsweeps` red-black sweeps time-skewed over plane slabs (the level stored by colour, one box; a slab is served
 * from the Infinity Cache from its second pass on), about `nlaunch` passes in all; avg_ms = time per pass over the whole level, cells = 0 when the level has no slab
 * schedule (smaller than 2^23 cells, several boxes, periodic faces).  bench.py: roofline.in_solve_ms_per_level_pass                                              */
int  vdn_bench_cc_smoother_in_solve(vdn_multifab *rh, vdn_multifab *phi, vdn_multifab **beta, const vdn_multifab *rho, const double *dx,
                                    const int *bc, int nsweeps, int nlaunch, double *avg_ms, long *cells);

#ifdef __cplusplus
}
#endif
#endif /* VARDEN_AMD_H */
