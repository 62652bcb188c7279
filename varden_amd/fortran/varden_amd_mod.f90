! varden_amd_mod.f90 -- Fortran (ISO_C_BINDING) host side of the MI355X-native VARDEN hot path.
!
! This is the module a VARDEN maintainer `use`s instead of the reference's
!     advance_module (src/advance_timestep.f90), estdt_module (src/estdt.f90),
!     hgproject_module (src/hgproject.f90) and of the FBoxLib containers those take
!     (multifab_module, ml_layout_module, define_bc_module).
! Names, argument order and meaning follow the reference; every routine forwards to the C-ABI of
! include/varden_amd.h (libvarden_amd.so, hand-written HIP for gfx950).  All multifab data lives in
! HBM: `dataptr` returns the DEVICE address (type(c_ptr)); use multifab_copy_to_host /
! multifab_copy_from_host for host access.  A non-zero C return code becomes `error stop` with the
! library's message (the reference calls bl_error, e.g. src/hgproject.f90:502).
!
! Differences from the reference that a caller sees:
!   * boxes are 0-based index boxes (lo(3), hi(3)) as in BoxLib; components are 1-based here
!     (Fortran side) and converted to the C-ABI's 0-based components inside this module;
!   * only dm = 3 and single-level hierarchies are implemented in this round.
module varden_amd
  use iso_c_binding
  implicit none
  private

  integer, parameter, public :: dp_t = c_double

  ! bc_module constants
  integer, parameter, public :: PERIODIC = -1, INTERIOR = 0, INLET = 11, OUTLET = 12, SYMMETRY = 13, &
                                SLIP_WALL = 14, NO_SLIP_WALL = 15
  integer, parameter, public :: REFLECT_ODD = 20, REFLECT_EVEN = 21, FOEXTRAP = 22, EXT_DIR = 23, HOEXTRAP = 24
  integer, parameter, public :: BC_PER = -1, BC_INT = 0, BC_DIR = 1, BC_NEU = 2
  ! proj_parameters (src/proj_parameters.f90)
  integer, parameter, public :: initial_projection = 1, divu_iters = 2, pressure_iters = 3, regular_timestep = 4

  ! mirror of vdn_params (include/varden_amd.h) == the probin_module values the hot path reads
  type, bind(C), public :: vdn_params
     integer(c_int) :: dm, nscal, slope_order, use_minion, boussinesq, stencil_order, diffusion_type
     integer(c_int) :: verbose, mg_verbose, prob_type
     real(c_double) :: visc_coef, diff_coef, cflfac, max_dt_growth
     real(c_double) :: u_bc(2,3), v_bc(2,3), w_bc(2,3), rho_bc(2,3), trac_bc(2,3)   ! C [dir][side] == Fortran (side,dir)
     integer(c_int) :: mg_nu1, mg_nu2, mg_nub, mg_max_iter, hg_max_iter, hg_nu1, hg_nu2, hg_nub
     real(c_double) :: hg_omega, mac_rel_eps, hg_rel_eps
     integer(c_int) :: abort_on_max_iter, hg_fmg, mac_fmg
     real(c_double) :: hg_omega_pre1, hg_omega_pre2, hg_omega_fac1, hg_omega_fac2, hg_omega_fac3
     integer(c_int) :: mg_predict
     integer(c_int) :: mg_bottom_solver, hg_bottom_solver, max_mg_bottom_nlevels      ! src/_parameters:55-57 (-1, 0, 4: bottom sweeps; 1, 3: BiCGStab; 2: CG; max_mg_bottom_nlevels has no effect)
     real(c_double) :: mg_bottom_solver_eps, hg_bottom_solver_eps                     ! 1e-3 (mac_multigrid.f90:56); the nodal one is ours
  end type vdn_params

  type, bind(C), public :: vdn_box
     integer(c_int) :: lo(3), hi(3)
  end type vdn_box

  ! refinement criteria chosen at run time (include/varden_amd.h: vdn_tag_criterion): a cell of level lev is tagged when gt(lev) < value < lt(lev) for ANY
  ! criterion; comp is 0-based here, as in C (make_tag_criterion takes the 1-based one)
  integer, parameter, public :: VDN_TAG_SCALAR = 0, VDN_TAG_SCALAR_GRAD = 1, VDN_TAG_VORTICITY = 2, VDN_TAG_MAGVEL = 3, VDN_TAG_MAX_CRITERIA = 8, VDN_MAXLEV = 4
  type, bind(C), public :: vdn_tag_criterion
     integer(c_int) :: field, comp
     real(c_double) :: gt(4), lt(4)
  end type vdn_tag_criterion

  ! run diagnostics over the composite grid (include/varden_amd.h: vdn_diag, vdn_diagnostics): counts, integrals (every cell weighted by its own volume), exact
  ! extrema; entries beyond nscal, dm or the levels of the hierarchy are 0.  VDN_DIAG_VORT: the vorticity terms (they read one ghost layer of u)
  integer, parameter, public :: VDN_DIAG_VORT = 1
  type, bind(C), public :: vdn_diag
     integer(c_long_long) :: cells, cells_lev(4), nonfinite
     real(c_double) :: volume, volume_lev(4)
     real(c_double) :: sum_s(11), momentum(3), kinetic, enstrophy
     real(c_double) :: s_min(11), s_max(11), u_min(3), u_max(3), magvel_max, vort_min, vort_max
  end type vdn_diag

  ! plane-averaged profiles along one axis (include/varden_amd.h: vdn_profile_layout, vdn_profiles): the number of rows of the result and the first row (0-based,
  ! as the library counts them; row r is out(:, r + 1)) of every row group
  type, bind(C), public :: vdn_profile_layout
     integer(c_int) :: nrow, volume, s, ss, u, ru, ruu, sua, s_min, s_max, u_min, u_max
  end type vdn_profile_layout

  ! what vdn_isosurface reports (include/varden_amd.h: vdn_iso): triangle and cut-cell counts, their parts per level, area, area vector, volumes
  type, bind(C), public :: vdn_iso
     integer(c_long_long) :: ntri, ntri_lev(4), cut_cells, cut_cells_lev(4), nonfinite_cells, written
     real(c_double) :: area, area_lev(4), area_vec(3), volume_above, volume
  end type vdn_iso

  type, public :: ml_layout
     type(c_ptr) :: h = c_null_ptr
     integer :: nlevel = 0, dim = 3
  end type ml_layout

  type, public :: multifab
     type(c_ptr) :: h = c_null_ptr
     integer :: dim = 3, nc = 1, ng = 0
  end type multifab

  type, public :: bc_tower
     type(c_ptr) :: h = c_null_ptr
  end type bc_tower

  ! Lagrangian tracer particles on the device (include/varden_amd.h: vdn_particles_*; DESIGN section 21); n: their number
  type, public :: particles
     type(c_ptr) :: h = c_null_ptr
     integer :: n = 0
  end type particles

  public :: varden_amd_initialize, varden_amd_finalize, probin_defaults, varden_amd_set_extruded_2d
  public :: ml_layout_build, ml_layout_destroy
  public :: bc_tower_build, bc_tower_destroy
  public :: multifab_build, multifab_build_edge, multifab_build_nodal, multifab_destroy, nfabs, get_box, dataptr, &
            setval, multifab_copy_c, norm_inf, norm_inf_c, multifab_fill_boundary, multifab_physbc, &
            multifab_copy_to_host, multifab_copy_from_host, multifab_fab_size
  public :: advance_timestep, estdt, hgproject, macproject
  public :: ml_cc_restriction, ml_edge_restriction, multifab_fill_ghost_cells, create_umac_grown, ml_restrict_and_fill
  public :: fillpatch, ml_nodal_prolongation, multifab_copy_layouts, make_new_grids, make_vorticity, make_magvel
  public :: make_new_grids_by, tag_boxes_by, make_tag_criterion
  public :: diagnostics
  public :: profiles_layout, profiles_nbins, profiles
  public :: isosurface, isosurface_write
  public :: sample_points, particles_create, particles_destroy, particles_count, particles_get, particles_advance, particles_sample, particles_write, particles_read
  public :: fabio_ml_multifab_write_d, fabio_ml_multifab_info, fabio_ml_multifab_boxes, fabio_ml_multifab_read_d, checkpoint_write, checkpoint_info
  public :: fabio_ml_multifab_write_plane_d, fabio_ml_multifab_read_plane_d, checkpoint_write_plane, make_vorticity_plane

  interface
     subroutine vdn_params_default(p) bind(C, name="vdn_params_default")
       import :: vdn_params
       type(vdn_params), intent(out) :: p
     end subroutine
     integer(c_int) function vdn_init(p, rank, nranks, device) bind(C, name="vdn_init")
       import :: vdn_params, c_int
       type(vdn_params), intent(in) :: p
       integer(c_int), value :: rank, nranks, device
     end function
     integer(c_int) function vdn_finalize() bind(C, name="vdn_finalize")
       import :: c_int
     end function
     integer(c_int) function vdn_set_extruded_2d(on) bind(C, name="vdn_set_extruded_2d")   ! a 2-D problem as its z-uniform 3-D copy: velpred_2d's hi-x OUTLET rule
       import :: c_int
       integer(c_int), value :: on
     end function
     type(c_ptr) function vdn_last_error() bind(C, name="vdn_last_error")
       import :: c_ptr
     end function
     integer(c_int) function vdn_layout_create(nlev, rr, pd, nboxes, boxes, owner, pmask, out) bind(C, name="vdn_layout_create")
       import :: c_int, c_ptr, vdn_box
       integer(c_int), value :: nlev
       integer(c_int), intent(in) :: rr(*), nboxes(*), owner(*), pmask(*)
       type(vdn_box), intent(in) :: pd(*), boxes(*)
       type(c_ptr), intent(out) :: out
     end function
     integer(c_int) function vdn_layout_destroy(la) bind(C, name="vdn_layout_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: la
     end function
     integer(c_int) function vdn_bc_tower_create(la, phys_bc, out) bind(C, name="vdn_bc_tower_create")
       import :: c_int, c_ptr
       type(c_ptr), value :: la
       integer(c_int), intent(in) :: phys_bc(*)
       type(c_ptr), intent(out) :: out
     end function
     integer(c_int) function vdn_bc_tower_destroy(b) bind(C, name="vdn_bc_tower_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: b
     end function
     integer(c_int) function vdn_multifab_create(la, lev, nc, ng, nodal, out) bind(C, name="vdn_multifab_create")
       import :: c_int, c_ptr
       type(c_ptr), value :: la
       integer(c_int), value :: lev, nc, ng
       integer(c_int), intent(in) :: nodal(3)
       type(c_ptr), intent(out) :: out
     end function
     integer(c_int) function vdn_multifab_destroy(mf) bind(C, name="vdn_multifab_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: mf
     end function
     integer(c_int) function vdn_multifab_nfabs(mf) bind(C, name="vdn_multifab_nfabs")
       import :: c_int, c_ptr
       type(c_ptr), value :: mf
     end function
     integer(c_int) function vdn_multifab_get_box(mf, i, bx) bind(C, name="vdn_multifab_get_box")
       import :: c_int, c_ptr, vdn_box
       type(c_ptr), value :: mf
       integer(c_int), value :: i
       type(vdn_box), intent(out) :: bx
     end function
     integer(c_long) function vdn_multifab_fab_size(mf, i) bind(C, name="vdn_multifab_fab_size")
       import :: c_int, c_long, c_ptr
       type(c_ptr), value :: mf
       integer(c_int), value :: i
     end function
     integer(c_int) function vdn_multifab_dataptr(mf, i, dev) bind(C, name="vdn_multifab_dataptr")
       import :: c_int, c_ptr
       type(c_ptr), value :: mf
       integer(c_int), value :: i
       type(c_ptr), intent(out) :: dev
     end function
     integer(c_int) function vdn_multifab_copy_to_host(mf, i, host) bind(C, name="vdn_multifab_copy_to_host")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: mf
       integer(c_int), value :: i
       real(c_double), intent(out) :: host(*)
     end function
     integer(c_int) function vdn_multifab_copy_from_host(mf, i, host) bind(C, name="vdn_multifab_copy_from_host")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: mf
       integer(c_int), value :: i
       real(c_double), intent(in) :: host(*)
     end function
     integer(c_int) function vdn_multifab_setval(mf, val, comp, nc, all) bind(C, name="vdn_multifab_setval")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: mf
       real(c_double), value :: val
       integer(c_int), value :: comp, nc, all
     end function
     integer(c_int) function vdn_multifab_copy_c(dst, dcomp, src, scomp, nc, ng) bind(C, name="vdn_multifab_copy_c")
       import :: c_int, c_ptr
       type(c_ptr), value :: dst, src
       integer(c_int), value :: dcomp, scomp, nc, ng
     end function
     integer(c_int) function vdn_multifab_norm_inf(mf, comp, nc, out) bind(C, name="vdn_multifab_norm_inf")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: mf
       integer(c_int), value :: comp, nc
       real(c_double), intent(out) :: out
     end function
     integer(c_int) function vdn_multifab_fill_boundary(mf) bind(C, name="vdn_multifab_fill_boundary")
       import :: c_int, c_ptr
       type(c_ptr), value :: mf
     end function
     integer(c_int) function vdn_multifab_physbc(mf, scomp, bccomp, nc, bct) bind(C, name="vdn_multifab_physbc")
       import :: c_int, c_ptr
       type(c_ptr), value :: mf, bct
       integer(c_int), value :: scomp, bccomp, nc
     end function
     integer(c_int) function vdn_advance_timestep(istep, mla, sold, uold, snew, unew, gp, p, evf, esf, bct, dt, time, dx, &
                                                  press_comp, proj_type) bind(C, name="vdn_advance_timestep")
       import :: c_int, c_ptr, c_double
       integer(c_int), value :: istep, press_comp, proj_type
       type(c_ptr), value :: mla, bct
       type(c_ptr), intent(in) :: sold(*), uold(*), snew(*), unew(*), gp(*), p(*), evf(*), esf(*)
       real(c_double), value :: dt, time
       real(c_double), intent(in) :: dx(*)
     end function
     integer(c_int) function vdn_estdt(lev, u, s, gp, evf, dx, dtold, dt) bind(C, name="vdn_estdt")
       import :: c_int, c_ptr, c_double
       integer(c_int), value :: lev
       type(c_ptr), value :: u, s, gp, evf
       real(c_double), intent(in) :: dx(3)
       real(c_double), value :: dtold
       real(c_double), intent(out) :: dt
     end function
     integer(c_int) function vdn_hgproject(proj_type, mla, unew, uold, rhohalf, p, gp, dx, dt, bct, press_comp) &
                                           bind(C, name="vdn_hgproject")
       import :: c_int, c_ptr, c_double
       integer(c_int), value :: proj_type, press_comp
       type(c_ptr), value :: mla, bct
       type(c_ptr), intent(in) :: unew(*), uold(*), rhohalf(*), p(*), gp(*)
       real(c_double), intent(in) :: dx(*)
       real(c_double), value :: dt
     end function
     integer(c_int) function vdn_macproject(mla, umac, rho, mac_rhs, dx, bct, bc_comp) bind(C, name="vdn_macproject")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: mla, bct
       type(c_ptr), intent(in) :: umac(*), rho(*), mac_rhs(*)
       real(c_double), intent(in) :: dx(*)
       integer(c_int), value :: bc_comp
     end function
     integer(c_int) function vdn_ml_cc_restriction(crse, fine, icomp, nc) bind(C, name="vdn_ml_cc_restriction")
       import :: c_int, c_ptr
       type(c_ptr), value :: crse, fine
       integer(c_int), value :: icomp, nc
     end function
     integer(c_int) function vdn_ml_edge_restriction(crse, fine, dir) bind(C, name="vdn_ml_edge_restriction")
       import :: c_int, c_ptr
       type(c_ptr), value :: crse, fine
       integer(c_int), value :: dir
     end function
     integer(c_int) function vdn_multifab_fill_ghost_cells(fine, crse, icomp, nc) bind(C, name="vdn_multifab_fill_ghost_cells")
       import :: c_int, c_ptr
       type(c_ptr), value :: fine, crse
       integer(c_int), value :: icomp, nc
     end function
     integer(c_int) function vdn_create_umac_grown(fine, crse, dir) bind(C, name="vdn_create_umac_grown")
       import :: c_int, c_ptr
       type(c_ptr), value :: fine, crse
       integer(c_int), value :: dir
     end function
     integer(c_int) function vdn_ml_restrict_and_fill(nlev, mf, icomp, bcomp, nc, same_boundary, bct) bind(C, name="vdn_ml_restrict_and_fill")
       import :: c_int, c_ptr
       integer(c_int), value :: nlev, icomp, bcomp, nc, same_boundary
       type(c_ptr), intent(in) :: mf(*)
       type(c_ptr), value :: bct
     end function
     integer(c_int) function vdn_fillpatch(fine, crse, icomp, nc) bind(C, name="vdn_fillpatch")
       import :: c_int, c_ptr
       type(c_ptr), value :: fine, crse
       integer(c_int), value :: icomp, nc
     end function
     integer(c_int) function vdn_make_vorticity(vort, comp, u, dx, bct) bind(C, name="vdn_make_vorticity")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: vort, u, bct
       integer(c_int), value :: comp
       real(c_double), intent(in) :: dx(*)
     end function
     integer(c_int) function vdn_make_magvel(magvel, comp, u) bind(C, name="vdn_make_magvel")
       import :: c_int, c_ptr
       type(c_ptr), value :: magvel, u
       integer(c_int), value :: comp
     end function
     integer(c_int) function vdn_ml_nodal_prolongation(fine, crse) bind(C, name="vdn_ml_nodal_prolongation")
       import :: c_int, c_ptr
       type(c_ptr), value :: fine, crse
     end function
     integer(c_int) function vdn_multifab_copy_layouts(dst, dcomp, src, scomp, nc) bind(C, name="vdn_multifab_copy_layouts")
       import :: c_int, c_ptr
       type(c_ptr), value :: dst, src
       integer(c_int), value :: dcomp, scomp, nc
     end function
     integer(c_int) function vdn_make_new_grids(s, lev1, buf_wid, nest, min_eff, min_width, blocking, max_grid_size, maxboxes, boxes_out, &
                                                nboxes_out, ntagged) bind(C, name="vdn_make_new_grids")
       import :: c_int, c_ptr, c_double, c_long, vdn_box
       type(c_ptr), value :: s
       integer(c_int), value :: lev1, buf_wid, nest, min_width, blocking, max_grid_size, maxboxes
       real(c_double), value :: min_eff
       type(vdn_box), intent(out) :: boxes_out(*)
       integer(c_int), intent(out) :: nboxes_out
       integer(c_long), intent(out) :: ntagged
     end function
     integer(c_int) function vdn_make_new_grids_by(s, u, dx, bct, lev1, ncrit, crit, buf_wid, nest, min_eff, min_width, blocking, max_grid_size, maxboxes, &
                                                   boxes_out, nboxes_out, ntagged) bind(C, name="vdn_make_new_grids_by")
       import :: c_int, c_ptr, c_double, c_long, vdn_box, vdn_tag_criterion
       type(c_ptr), value :: s, u, bct
       real(c_double), intent(in) :: dx(*)
       integer(c_int), value :: lev1, ncrit, buf_wid, nest, min_width, blocking, max_grid_size, maxboxes
       type(vdn_tag_criterion), intent(in) :: crit(*)
       real(c_double), value :: min_eff
       type(vdn_box), intent(out) :: boxes_out(*)
       integer(c_int), intent(out) :: nboxes_out
       integer(c_long), intent(out) :: ntagged
     end function
     integer(c_int) function vdn_tag_boxes_by(s, u, dx, bct, lev1, ncrit, crit, tags_host) bind(C, name="vdn_tag_boxes_by")
       import :: c_int, c_ptr, c_double, c_signed_char, vdn_tag_criterion
       type(c_ptr), value :: s, u, bct
       real(c_double), intent(in) :: dx(*)
       integer(c_int), value :: lev1, ncrit
       type(vdn_tag_criterion), intent(in) :: crit(*)
       integer(c_signed_char), intent(out) :: tags_host(*)
     end function
     integer(c_int) function vdn_diagnostics(nlev, mla, u, s, dx, bct, what, out) bind(C, name="vdn_diagnostics")
       import :: c_int, c_ptr, c_double, vdn_diag
       integer(c_int), value :: nlev, what
       type(c_ptr), value :: mla, bct
       type(c_ptr), intent(in) :: u(*), s(*)
       real(c_double), intent(in) :: dx(*)
       type(vdn_diag), intent(out) :: out
     end function
     integer(c_size_t) function vdn_diag_sizeof() bind(C, name="vdn_diag_sizeof")
       import :: c_size_t
     end function
     integer(c_int) function vdn_profiles_layout(dm, nscal, lay) bind(C, name="vdn_profiles_layout")
       import :: c_int, vdn_profile_layout
       integer(c_int), value :: dm, nscal
       type(vdn_profile_layout), intent(out) :: lay
     end function
     integer(c_size_t) function vdn_profile_layout_sizeof() bind(C, name="vdn_profile_layout_sizeof")
       import :: c_size_t
     end function
     integer(c_long) function vdn_profiles_nbins(nlev, mla, axis) bind(C, name="vdn_profiles_nbins")
       import :: c_int, c_long, c_ptr
       integer(c_int), value :: nlev, axis
       type(c_ptr), value :: mla
     end function
     integer(c_int) function vdn_profiles(nlev, mla, u, s, dx, axis, nbins, out_host, cells_host) bind(C, name="vdn_profiles")
       import :: c_int, c_long, c_long_long, c_ptr, c_double
       integer(c_int), value :: nlev, axis
       integer(c_long), value :: nbins
       type(c_ptr), value :: mla
       type(c_ptr), intent(in) :: u(*), s(*)
       real(c_double), intent(in) :: dx(*)
       real(c_double), intent(out) :: out_host(*)
       integer(c_long_long), intent(out) :: cells_host(*)
     end function
     ! isosurfaces (include/varden_amd.h; csrc/iso.hip): tri_host and lev_host are addresses, c_null_ptr for "none"
     integer(c_size_t) function vdn_iso_sizeof() bind(C, name="vdn_iso_sizeof")
       import :: c_size_t
     end function
     integer(c_int) function vdn_isosurface(nlev, mla, mf, comp, bccomp, dx, bct, iso, max_tri, tri_host, lev_host, out) bind(C, name="vdn_isosurface")
       import :: c_int, c_long_long, c_ptr, c_double, vdn_iso
       integer(c_int), value :: nlev, comp, bccomp
       type(c_ptr), value :: mla, bct, tri_host, lev_host
       type(c_ptr), intent(in) :: mf(*)
       real(c_double), intent(in) :: dx(*)
       real(c_double), value :: iso
       integer(c_long_long), value :: max_tri
       type(vdn_iso), intent(out) :: out
     end function
     integer(c_int) function vdn_isosurface_write(path, ntri, tri_host, lev_host, iso, time) bind(C, name="vdn_isosurface_write")
       import :: c_int, c_long_long, c_ptr, c_double, c_char
       character(kind=c_char), intent(in) :: path(*)
       integer(c_long_long), value :: ntri
       type(c_ptr), value :: tri_host, lev_host
       real(c_double), value :: iso, time
     end function
     ! values at points and tracer particles (include/varden_amd.h; csrc/particles.hip)
     integer(c_int) function vdn_sample_points(nlev, mla, mf, comp, nc, bccomp, dx, bct, n, x_host, val_host, lev_host) bind(C, name="vdn_sample_points")
       import :: c_int, c_ptr, c_double, c_long
       integer(c_int), value :: nlev, comp, nc, bccomp
       type(c_ptr), value :: mla, bct
       type(c_ptr), intent(in) :: mf(*)
       real(c_double), intent(in) :: dx(*), x_host(*)
       integer(c_long), value :: n
       real(c_double), intent(out) :: val_host(*)
       integer(c_int), intent(out) :: lev_host(*)
     end function
     integer(c_int) function vdn_particles_create(n, x_host, P) bind(C, name="vdn_particles_create")
       import :: c_int, c_ptr, c_double, c_long
       integer(c_long), value :: n
       real(c_double), intent(in) :: x_host(*)
       type(c_ptr), intent(out) :: P
     end function
     integer(c_int) function vdn_particles_destroy(P) bind(C, name="vdn_particles_destroy")
       import :: c_int, c_ptr
       type(c_ptr), value :: P
     end function
     integer(c_int) function vdn_particles_count(P, n, active) bind(C, name="vdn_particles_count")
       import :: c_int, c_ptr, c_long
       type(c_ptr), value :: P
       integer(c_long), intent(out) :: n, active
     end function
     integer(c_int) function vdn_particles_get(P, x_host, state_host) bind(C, name="vdn_particles_get")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: P
       real(c_double), intent(out) :: x_host(*)
       integer(c_int), intent(out) :: state_host(*)
     end function
     integer(c_int) function vdn_particles_advance(P, nlev, mla, u0, u1, dx, bct, dt) bind(C, name="vdn_particles_advance")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: P, mla, bct
       integer(c_int), value :: nlev
       type(c_ptr), intent(in) :: u0(*), u1(*)
       real(c_double), intent(in) :: dx(*)
       real(c_double), value :: dt
     end function
     integer(c_int) function vdn_particles_sample(P, nlev, mla, mf, comp, nc, bccomp, dx, bct, val_host, lev_host) bind(C, name="vdn_particles_sample")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: P, mla, bct
       integer(c_int), value :: nlev, comp, nc, bccomp
       type(c_ptr), intent(in) :: mf(*)
       real(c_double), intent(in) :: dx(*)
       real(c_double), intent(out) :: val_host(*)
       integer(c_int), intent(out) :: lev_host(*)
     end function
     integer(c_int) function vdn_particles_write(P, path, time, ncol, names, cols) bind(C, name="vdn_particles_write")
       import :: c_int, c_ptr, c_double, c_char
       type(c_ptr), value :: P
       character(kind=c_char), intent(in) :: path(*)
       real(c_double), value :: time
       integer(c_int), value :: ncol
       type(c_ptr), intent(in) :: names(*)
       real(c_double), intent(in) :: cols(*)
     end function
     integer(c_int) function vdn_particles_read(path, P, time) bind(C, name="vdn_particles_read")
       import :: c_int, c_ptr, c_double, c_char
       character(kind=c_char), intent(in) :: path(*)
       type(c_ptr), intent(out) :: P
       real(c_double), intent(out) :: time
     end function
     ! plot files and checkpoints inside the library (include/varden_amd.h; csrc/fabio.hip); optional C arguments travel as addresses (c_null_ptr: the default)
     integer(c_int) function vdn_fabio_ml_multifab_write_d(dirname, nlev, mfs, rr, names, pd0, prob_lo, prob_hi, time, dx0, staging_bytes) &
                                                           bind(C, name="vdn_fabio_ml_multifab_write_d")
       import :: c_int, c_ptr, c_char, c_double, c_long
       character(kind=c_char), intent(in) :: dirname(*)
       integer(c_int), value :: nlev
       type(c_ptr), intent(in) :: mfs(*)
       integer(c_int), intent(in) :: rr(*)
       type(c_ptr), value :: names, pd0, prob_lo, prob_hi, dx0
       real(c_double), value :: time
       integer(c_long), value :: staging_bytes
     end function
     integer(c_int) function vdn_fabio_ml_multifab_info(dirname, nlev, dm, ncomp, nodal, nboxes, rr, time) bind(C, name="vdn_fabio_ml_multifab_info")
       import :: c_int, c_char, c_double
       character(kind=c_char), intent(in) :: dirname(*)
       integer(c_int), intent(out) :: nlev, dm, ncomp, nodal(3), nboxes(*), rr(*)
       real(c_double), intent(out) :: time
     end function
     integer(c_int) function vdn_fabio_ml_multifab_boxes(dirname, lev, boxes, maxboxes) bind(C, name="vdn_fabio_ml_multifab_boxes")
       import :: c_int, c_char, vdn_box
       character(kind=c_char), intent(in) :: dirname(*)
       integer(c_int), value :: lev, maxboxes
       type(vdn_box), intent(out) :: boxes(*)
     end function
     integer(c_int) function vdn_fabio_ml_multifab_read_d(dirname, nlev, mfs, staging_bytes) bind(C, name="vdn_fabio_ml_multifab_read_d")
       import :: c_int, c_ptr, c_char, c_long
       character(kind=c_char), intent(in) :: dirname(*)
       integer(c_int), value :: nlev
       type(c_ptr), intent(in) :: mfs(*)
       integer(c_long), value :: staging_bytes
     end function
     integer(c_int) function vdn_checkpoint_write(dirname, nlev, state, pressure, rr, time, dt, staging_bytes) bind(C, name="vdn_checkpoint_write")
       import :: c_int, c_ptr, c_char, c_double, c_long
       character(kind=c_char), intent(in) :: dirname(*)
       integer(c_int), value :: nlev
       type(c_ptr), intent(in) :: state(*), pressure(*)
       integer(c_int), intent(in) :: rr(*)
       real(c_double), value :: time, dt
       integer(c_long), value :: staging_bytes
     end function
     integer(c_int) function vdn_checkpoint_info(dirname, nlev, time, dt, rr) bind(C, name="vdn_checkpoint_info")
       import :: c_int, c_char, c_double
       character(kind=c_char), intent(in) :: dirname(*)
       integer(c_int), intent(out) :: nlev, rr(*)
       real(c_double), intent(out) :: time, dt
     end function
     ! the same files for a 2-D problem run as its z-uniform 3-D copy: plane k = 0 as a dm = 2 hierarchy (include/varden_amd.h)
     integer(c_int) function vdn_fabio_ml_multifab_write_plane_d(dirname, nlev, mfs, rr, names, pd0, prob_lo, prob_hi, time, dx0, staging_bytes, ncomp, comps, &
                                                                 nvanish, vanish, defect) bind(C, name="vdn_fabio_ml_multifab_write_plane_d")
       import :: c_int, c_ptr, c_char, c_double, c_long
       character(kind=c_char), intent(in) :: dirname(*)
       integer(c_int), value :: nlev, ncomp, nvanish
       type(c_ptr), intent(in) :: mfs(*)
       integer(c_int), intent(in) :: rr(*), comps(*), vanish(*)
       type(c_ptr), value :: names, pd0, prob_lo, prob_hi, dx0, defect
       real(c_double), value :: time
       integer(c_long), value :: staging_bytes
     end function
     integer(c_int) function vdn_fabio_ml_multifab_read_plane_d(dirname, nlev, mfs, staging_bytes, ncomp, comps) bind(C, name="vdn_fabio_ml_multifab_read_plane_d")
       import :: c_int, c_ptr, c_char, c_long
       character(kind=c_char), intent(in) :: dirname(*)
       integer(c_int), value :: nlev, ncomp
       type(c_ptr), intent(in) :: mfs(*)
       integer(c_long), value :: staging_bytes
       integer(c_int), intent(in) :: comps(*)
     end function
     integer(c_int) function vdn_checkpoint_write_plane(dirname, nlev, state, pressure, rr, time, dt, staging_bytes, ncomp, comps, nvanish, vanish, defect) &
                                                        bind(C, name="vdn_checkpoint_write_plane")
       import :: c_int, c_ptr, c_char, c_double, c_long
       character(kind=c_char), intent(in) :: dirname(*)
       integer(c_int), value :: nlev, ncomp, nvanish
       type(c_ptr), intent(in) :: state(*), pressure(*)
       integer(c_int), intent(in) :: rr(*), comps(*), vanish(*)
       real(c_double), value :: time, dt
       integer(c_long), value :: staging_bytes
       real(c_double), intent(out) :: defect(2)
     end function
     integer(c_int) function vdn_make_vorticity_plane(vort, comp, u, dx, bct) bind(C, name="vdn_make_vorticity_plane")
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: vort, u, bct
       integer(c_int), value :: comp
       real(c_double), intent(in) :: dx(*)
     end function
     integer(c_int) function vdn_last_bottom_form(which) bind(C, name="vdn_last_bottom_form")   ! 0 bottom sweeps, 1 Krylov in one workgroup, 2 Krylov over the whole GPU
       import :: c_int
       integer(c_int), value :: which
     end function
     integer(c_size_t) function c_strlen(s) bind(C, name="strlen")
       import :: c_ptr, c_size_t
       type(c_ptr), value :: s
     end function
  end interface

contains

  ! ---- error convention: non-zero return => error stop with the library's message ----------------
  subroutine chk(rc, where)
    integer(c_int), intent(in) :: rc
    character(len=*), intent(in) :: where
    type(c_ptr) :: msg
    character(kind=c_char), pointer :: s(:)
    integer :: n, i
    character(len=512) :: buf
    if (rc == 0) return
    msg = vdn_last_error()
    n = int(c_strlen(msg))
    call c_f_pointer(msg, s, [n])
    buf = ' '
    do i = 1, min(n, 512)
       buf(i:i) = s(i)
    end do
    write(*,*) 'varden_amd: ', where, ': ', trim(buf)
    error stop 1
  end subroutine chk

  subroutine probin_defaults(p)
    type(vdn_params), intent(out) :: p
    call vdn_params_default(p)
  end subroutine probin_defaults

  subroutine varden_amd_initialize(p, rank, nranks, device)
    type(vdn_params), intent(in) :: p
    integer, intent(in) :: rank, nranks, device
    call chk(vdn_init(p, int(rank, c_int), int(nranks, c_int), int(device, c_int)), 'vdn_init')
  end subroutine varden_amd_initialize

  ! the 3-D kernels run a z-uniform copy of a 2-D problem: velpred_2d's hi-x OUTLET rule (include/varden_amd.h: vdn_set_extruded_2d); after varden_amd_initialize
  subroutine varden_amd_set_extruded_2d(on)
    logical, intent(in) :: on
    call chk(vdn_set_extruded_2d(merge(1_c_int, 0_c_int, on)), 'vdn_set_extruded_2d')
  end subroutine varden_amd_set_extruded_2d

  subroutine varden_amd_finalize()
    call chk(vdn_finalize(), 'vdn_finalize')
  end subroutine varden_amd_finalize

  ! ---- ml_layout -------------------------------------------------------------------------------------
  subroutine ml_layout_build(mla, nlev, rr, pd, nboxes, boxes, owner, pmask)
    type(ml_layout), intent(out) :: mla
    integer, intent(in) :: nlev, rr(:), nboxes(:), owner(:)
    type(vdn_box), intent(in) :: pd(:), boxes(:)
    logical, intent(in) :: pmask(3)
    integer(c_int) :: pm(3)
    pm = merge(1, 0, pmask)
    call chk(vdn_layout_create(int(nlev, c_int), int(rr, c_int), pd, int(nboxes, c_int), boxes, int(owner, c_int), pm, mla%h), &
             'ml_layout_build')
    mla%nlevel = nlev
    mla%dim = 3
  end subroutine ml_layout_build

  subroutine ml_layout_destroy(mla)
    type(ml_layout), intent(inout) :: mla
    call chk(vdn_layout_destroy(mla%h), 'ml_layout_destroy')
    mla%h = c_null_ptr
  end subroutine ml_layout_destroy

  ! ---- bc_tower (define_bc_tower.f90): phys_bc(dir, side) as in the reference ---------------------------
  subroutine bc_tower_build(bct, mla, phys_bc)
    type(bc_tower), intent(out) :: bct
    type(ml_layout), intent(in) :: mla
    integer, intent(in) :: phys_bc(3, 2)
    integer(c_int) :: flat(6)
    integer :: d, s
    do d = 1, 3
       do s = 1, 2
          flat((d - 1) * 2 + s) = phys_bc(d, s)
       end do
    end do
    call chk(vdn_bc_tower_create(mla%h, flat, bct%h), 'bc_tower_build')
  end subroutine bc_tower_build

  subroutine bc_tower_destroy(bct)
    type(bc_tower), intent(inout) :: bct
    call chk(vdn_bc_tower_destroy(bct%h), 'bc_tower_destroy')
    bct%h = c_null_ptr
  end subroutine bc_tower_destroy

  ! ---- multifab ---------------------------------------------------------------------------------------
  subroutine multifab_build(mf, mla, lev, nc, ng)
    type(multifab), intent(out) :: mf
    type(ml_layout), intent(in) :: mla
    integer, intent(in) :: lev, nc, ng
    integer(c_int) :: nodal(3)
    nodal = 0
    call chk(vdn_multifab_create(mla%h, int(lev - 1, c_int), int(nc, c_int), int(ng, c_int), nodal, mf%h), 'multifab_build')
    mf%nc = nc; mf%ng = ng
  end subroutine multifab_build

  subroutine multifab_build_edge(mf, mla, lev, nc, ng, dir)
    type(multifab), intent(out) :: mf
    type(ml_layout), intent(in) :: mla
    integer, intent(in) :: lev, nc, ng, dir
    integer(c_int) :: nodal(3)
    nodal = 0
    nodal(dir) = 1
    call chk(vdn_multifab_create(mla%h, int(lev - 1, c_int), int(nc, c_int), int(ng, c_int), nodal, mf%h), 'multifab_build_edge')
    mf%nc = nc; mf%ng = ng
  end subroutine multifab_build_edge

  subroutine multifab_build_nodal(mf, mla, lev, nc, ng)
    type(multifab), intent(out) :: mf
    type(ml_layout), intent(in) :: mla
    integer, intent(in) :: lev, nc, ng
    integer(c_int) :: nodal(3)
    nodal = 1
    call chk(vdn_multifab_create(mla%h, int(lev - 1, c_int), int(nc, c_int), int(ng, c_int), nodal, mf%h), 'multifab_build_nodal')
    mf%nc = nc; mf%ng = ng
  end subroutine multifab_build_nodal

  subroutine multifab_destroy(mf)
    type(multifab), intent(inout) :: mf
    call chk(vdn_multifab_destroy(mf%h), 'multifab_destroy')
    mf%h = c_null_ptr
  end subroutine multifab_destroy

  integer function nfabs(mf)
    type(multifab), intent(in) :: mf
    nfabs = vdn_multifab_nfabs(mf%h)
  end function nfabs

  function get_box(mf, i) result(bx)
    type(multifab), intent(in) :: mf
    integer, intent(in) :: i
    type(vdn_box) :: bx
    call chk(vdn_multifab_get_box(mf%h, int(i - 1, c_int), bx), 'get_box')
  end function get_box

  function dataptr(mf, i) result(dev)
    type(multifab), intent(in) :: mf
    integer, intent(in) :: i
    type(c_ptr) :: dev
    call chk(vdn_multifab_dataptr(mf%h, int(i - 1, c_int), dev), 'dataptr')
  end function dataptr

  integer(c_long) function multifab_fab_size(mf, i)
    type(multifab), intent(in) :: mf
    integer, intent(in) :: i
    multifab_fab_size = vdn_multifab_fab_size(mf%h, int(i - 1, c_int))
  end function multifab_fab_size

  subroutine multifab_copy_to_host(mf, i, host)
    type(multifab), intent(in) :: mf
    integer, intent(in) :: i
    real(dp_t), intent(out) :: host(*)
    call chk(vdn_multifab_copy_to_host(mf%h, int(i - 1, c_int), host), 'multifab_copy_to_host')
  end subroutine multifab_copy_to_host

  subroutine multifab_copy_from_host(mf, i, host)
    type(multifab), intent(inout) :: mf
    integer, intent(in) :: i
    real(dp_t), intent(in) :: host(*)
    call chk(vdn_multifab_copy_from_host(mf%h, int(i - 1, c_int), host), 'multifab_copy_from_host')
  end subroutine multifab_copy_from_host

  ! setval(mf, val, [comp, nc], [all])
  subroutine setval(mf, val, comp, nc, all)
    type(multifab), intent(inout) :: mf
    real(dp_t), intent(in) :: val
    integer, intent(in), optional :: comp, nc
    logical, intent(in), optional :: all
    integer :: c, n, a
    c = 1; if (present(comp)) c = comp
    n = mf%nc - c + 1; if (present(nc)) n = nc
    a = 0; if (present(all)) a = merge(1, 0, all)
    call chk(vdn_multifab_setval(mf%h, val, int(c - 1, c_int), int(n, c_int), int(a, c_int)), 'setval')
  end subroutine setval

  ! multifab_copy_c(dst, dcomp, src, scomp, nc, ng)
  subroutine multifab_copy_c(dst, dcomp, src, scomp, nc, ng)
    type(multifab), intent(inout) :: dst
    type(multifab), intent(in) :: src
    integer, intent(in) :: dcomp, scomp, nc
    integer, intent(in), optional :: ng
    integer :: g
    g = 0; if (present(ng)) g = ng
    call chk(vdn_multifab_copy_c(dst%h, int(dcomp - 1, c_int), src%h, int(scomp - 1, c_int), int(nc, c_int), int(g, c_int)), &
             'multifab_copy_c')
  end subroutine multifab_copy_c

  real(dp_t) function norm_inf(mf)
    type(multifab), intent(in) :: mf
    call chk(vdn_multifab_norm_inf(mf%h, 0_c_int, int(mf%nc, c_int), norm_inf), 'norm_inf')
  end function norm_inf
  ! norm_inf(mf, comp, nc)   (FBoxLib; src/advance_timestep.f90:187: the max norm of nc components from comp, 1-based)
  real(dp_t) function norm_inf_c(mf, comp, nc)
    type(multifab), intent(in) :: mf
    integer, intent(in) :: comp, nc
    call chk(vdn_multifab_norm_inf(mf%h, int(comp - 1, c_int), int(nc, c_int), norm_inf_c), 'norm_inf')
  end function norm_inf_c

  subroutine multifab_fill_boundary(mf)
    type(multifab), intent(inout) :: mf
    call chk(vdn_multifab_fill_boundary(mf%h), 'multifab_fill_boundary')
  end subroutine multifab_fill_boundary

  ! multifab_physbc(s, start_scomp, start_bccomp, num_comp, the_bc_tower)   (src/multifab_physbc.f90:17)
  subroutine multifab_physbc(s, start_scomp, start_bccomp, num_comp, the_bc_tower)
    type(multifab), intent(inout) :: s
    integer, intent(in) :: start_scomp, start_bccomp, num_comp
    type(bc_tower), intent(in) :: the_bc_tower
    call chk(vdn_multifab_physbc(s%h, int(start_scomp - 1, c_int), int(start_bccomp - 1, c_int), int(num_comp, c_int), &
             the_bc_tower%h), 'multifab_physbc')
  end subroutine multifab_physbc

  ! ---- the hot path: same argument list as reference src/advance_timestep.f90:26-44 ---------------------
  subroutine advance_timestep(istep, mla, sold, uold, snew, unew, gp, p, ext_vel_force, ext_scal_force, &
                              the_bc_tower, dt, time, dx, press_comp, proj_type)
    integer        , intent(in   ) :: istep
    type(ml_layout), intent(in   ) :: mla
    type(multifab) , intent(inout) :: sold(:), uold(:), snew(:), unew(:), gp(:), p(:)
    type(multifab) , intent(inout) :: ext_vel_force(:), ext_scal_force(:)
    real(dp_t)     , intent(in   ) :: dt, time, dx(:,:)
    type(bc_tower) , intent(in   ) :: the_bc_tower
    integer        , intent(in   ) :: press_comp, proj_type
    real(c_double) :: dxc(3 * size(dx, 1))
    integer :: n, d
    do n = 1, size(dx, 1)          ! dx(level, dir) -> C [level][dir]
       do d = 1, 3
          dxc((n - 1) * 3 + d) = dx(n, d)
       end do
    end do
    call chk(vdn_advance_timestep(int(istep, c_int), mla%h, handles(sold), handles(uold), handles(snew), handles(unew), &
                                  handles(gp), handles(p), handles(ext_vel_force), handles(ext_scal_force), the_bc_tower%h, &
                                  dt, time, dxc, int(press_comp, c_int), int(proj_type, c_int)), 'advance_timestep')
  end subroutine advance_timestep

  ! estdt(lev, u, s, gp, ext_vel_force, dx, dtold, dt)   (src/estdt.f90:15)
  subroutine estdt(lev, u, s, gp, ext_vel_force, dx, dtold, dt)
    integer        , intent(in ) :: lev
    type(multifab) , intent(in ) :: u, s, gp, ext_vel_force
    real(dp_t)     , intent(in ) :: dx(:), dtold
    real(dp_t)     , intent(out) :: dt
    real(c_double) :: dxc(3)
    dxc = dx(1:3)
    call chk(vdn_estdt(int(lev, c_int), u%h, s%h, gp%h, ext_vel_force%h, dxc, dtold, dt), 'estdt')
  end subroutine estdt

  ! hgproject(proj_type, mla, unew, uold, rhohalf, p, gp, dx, dt, the_bc_tower, press_comp)  (src/hgproject.f90:17)
  subroutine hgproject(proj_type, mla, unew, uold, rhohalf, p, gp, dx, dt, the_bc_tower, press_comp)
    integer        , intent(in   ) :: proj_type, press_comp
    type(ml_layout), intent(in   ) :: mla
    type(multifab) , intent(inout) :: unew(:), rhohalf(:), p(:), gp(:)
    type(multifab) , intent(in   ) :: uold(:)
    real(dp_t)     , intent(in   ) :: dx(:,:), dt
    type(bc_tower) , intent(in   ) :: the_bc_tower
    real(c_double) :: dxc(3 * size(dx, 1))
    integer :: n, d
    do n = 1, size(dx, 1)
       do d = 1, 3
          dxc((n - 1) * 3 + d) = dx(n, d)
       end do
    end do
    call chk(vdn_hgproject(int(proj_type, c_int), mla%h, handles(unew), handles(uold), handles(rhohalf), handles(p), &
                           handles(gp), dxc, dt, the_bc_tower%h, int(press_comp, c_int)), 'hgproject')
  end subroutine hgproject

  ! macproject(mla, umac, rho, dx, the_bc_tower, bc_comp, mac_rhs)  (src/macproject.f90:20); umac(n,d)
  subroutine macproject(mla, umac, rho, dx, the_bc_tower, bc_comp, mac_rhs)
    type(ml_layout), intent(in   ) :: mla
    type(multifab) , intent(inout) :: umac(:,:)
    type(multifab) , intent(in   ) :: rho(:), mac_rhs(:)
    real(dp_t)     , intent(in   ) :: dx(:,:)
    type(bc_tower) , intent(in   ) :: the_bc_tower
    integer        , intent(in   ) :: bc_comp
    real(c_double) :: dxc(3 * size(dx, 1))
    type(c_ptr) :: um(3 * size(umac, 1))
    integer :: n, d
    do n = 1, size(dx, 1)
       do d = 1, 3
          dxc((n - 1) * 3 + d) = dx(n, d)
          um((n - 1) * 3 + d) = umac(n, d)%h
       end do
    end do
    call chk(vdn_macproject(mla%h, um, handles(rho), handles(mac_rhs), dxc, the_bc_tower%h, int(bc_comp, c_int)), 'macproject')
  end subroutine macproject

  ! FBoxLib names; components 1-based as in the reference, rr is accepted for signature compatibility (ratio 2 only)
  subroutine ml_cc_restriction(crse, fine, rr)
    type(multifab), intent(inout) :: crse
    type(multifab), intent(in   ) :: fine
    integer       , intent(in   ) :: rr(:)
    call chk(vdn_ml_cc_restriction(crse%h, fine%h, 0_c_int, int(crse%nc, c_int)), 'ml_cc_restriction')
  end subroutine ml_cc_restriction
  subroutine ml_edge_restriction(crse, fine, rr, dir)
    type(multifab), intent(inout) :: crse
    type(multifab), intent(in   ) :: fine
    integer       , intent(in   ) :: rr(:), dir
    call chk(vdn_ml_edge_restriction(crse%h, fine%h, int(dir - 1, c_int)), 'ml_edge_restriction')
  end subroutine ml_edge_restriction
  subroutine multifab_fill_ghost_cells(fine, crse, icomp, nc)
    type(multifab), intent(inout) :: fine
    type(multifab), intent(in   ) :: crse
    integer       , intent(in   ) :: icomp, nc
    call chk(vdn_multifab_fill_ghost_cells(fine%h, crse%h, int(icomp - 1, c_int), int(nc, c_int)), 'multifab_fill_ghost_cells')
  end subroutine multifab_fill_ghost_cells
  subroutine create_umac_grown(fine, crse, dir)
    type(multifab), intent(inout) :: fine
    type(multifab), intent(in   ) :: crse
    integer       , intent(in   ) :: dir
    call chk(vdn_create_umac_grown(fine%h, crse%h, int(dir - 1, c_int)), 'create_umac_grown')
  end subroutine create_umac_grown
  subroutine ml_restrict_and_fill(nlevs, mf, the_bc_tower, icomp, bcomp, nc, same_boundary)
    integer       , intent(in   ) :: nlevs, icomp, bcomp, nc
    type(multifab), intent(inout) :: mf(:)
    type(bc_tower), intent(in   ) :: the_bc_tower
    logical       , intent(in   ) :: same_boundary
    call chk(vdn_ml_restrict_and_fill(int(nlevs, c_int), handles(mf), int(icomp - 1, c_int), int(bcomp - 1, c_int), int(nc, c_int), &
                                      merge(1_c_int, 0_c_int, same_boundary), the_bc_tower%h), 'ml_restrict_and_fill')
  end subroutine ml_restrict_and_fill

  ! fillpatch(fine, crse, 0, ...) / ml_nodal_prolongation / multifab_copy_c across box lists: src/regrid.f90:311-337
  subroutine fillpatch(fine, crse, icomp, nc)
    type(multifab), intent(inout) :: fine
    type(multifab), intent(in   ) :: crse
    integer       , intent(in   ) :: icomp, nc
    call chk(vdn_fillpatch(fine%h, crse%h, int(icomp - 1, c_int), int(nc, c_int)), 'fillpatch')
  end subroutine fillpatch
  ! vort_module (src/makevort.f90:16-91): the derived quantities of write_plotfile; bc is the tower, the level is u's
  subroutine make_vorticity(vort, comp, u, dx, the_bc_tower)
    type(multifab), intent(inout) :: vort, u
    integer       , intent(in   ) :: comp
    real(dp_t)    , intent(in   ) :: dx(:)
    type(bc_tower), intent(in   ) :: the_bc_tower
    real(c_double) :: d(3)
    d = 1.0_c_double; d(1:size(dx)) = dx
    call chk(vdn_make_vorticity(vort%h, int(comp - 1, c_int), u%h, d, the_bc_tower%h), 'make_vorticity')
  end subroutine make_vorticity
  ! makevort_2d's rule (src/makevort.f90:93-156) on every plane of a z-uniform 3-D copy; dx: the two in-plane spacings
  subroutine make_vorticity_plane(vort, comp, u, dx, the_bc_tower)
    type(multifab), intent(inout) :: vort, u
    integer       , intent(in   ) :: comp
    real(dp_t)    , intent(in   ) :: dx(:)
    type(bc_tower), intent(in   ) :: the_bc_tower
    real(c_double) :: d(3)
    d = 1.0_c_double; d(1:2) = dx(1:2)
    call chk(vdn_make_vorticity_plane(vort%h, int(comp - 1, c_int), u%h, d, the_bc_tower%h), 'make_vorticity_plane')
  end subroutine make_vorticity_plane
  ! run diagnostics of the state (u, s) of levels 1 .. size(u) over the composite grid: see vdn_diagnostics.  vort (default .true.): the vorticity terms too -- the
  ! CALLER has filled one ghost layer of u (same level, physical boundary, coarse-fine), as the drivers do at the top of every step; nothing is filled here
  subroutine diagnostics(mla, u, s, dx, the_bc_tower, diag, vort)
    type(ml_layout), intent(in   ) :: mla
    type(multifab) , intent(in   ) :: u(:), s(:)
    real(dp_t)     , intent(in   ) :: dx(:,:)
    type(bc_tower) , intent(in   ) :: the_bc_tower
    type(vdn_diag) , intent(  out) :: diag
    logical, intent(in), optional  :: vort
    real(c_double) :: dxc(3 * size(u))
    integer :: n, d
    integer(c_int) :: what
    if (vdn_diag_sizeof() /= c_sizeof(diag)) error stop 'diagnostics: vdn_diag differs between the library and this module'
    what = VDN_DIAG_VORT
    if (present(vort)) then
       if (.not. vort) what = 0
    end if
    dxc = 1.0_c_double
    do n = 1, size(u)
       do d = 1, min(3, size(dx, 2))
          dxc((n - 1) * 3 + d) = dx(n, d)
       end do
    end do
    call chk(vdn_diagnostics(int(size(u), c_int), mla%h, handles(u), handles(s), dxc, the_bc_tower%h, what, diag), 'diagnostics')
  end subroutine diagnostics
  ! plane-averaged profiles (see vdn_profiles): the offsets of the row groups for (dm, nscal) ...
  subroutine profiles_layout(dm, nscal, lay)
    integer, intent(in) :: dm, nscal
    type(vdn_profile_layout), intent(out) :: lay
    if (vdn_profile_layout_sizeof() /= c_sizeof(lay)) error stop 'profiles_layout: vdn_profile_layout differs between the library and this module'
    call chk(vdn_profiles_layout(int(dm, c_int), int(nscal, c_int), lay), 'profiles_layout')
  end subroutine profiles_layout
  ! ... the number of bins of a hierarchy of nlev levels along axis (1-based): the planes of its finest level ...
  function profiles_nbins(mla, nlev, axis) result(nbins)
    type(ml_layout), intent(in) :: mla
    integer, intent(in) :: nlev, axis
    integer :: nbins
    integer(c_long) :: n
    n = vdn_profiles_nbins(int(nlev, c_int), mla%h, int(axis - 1, c_int))
    if (n < 0) call chk(1_c_int, 'profiles_nbins')
    nbins = int(n)
  end function profiles_nbins
  ! ... and the profiles of the state (u, s) of levels 1 .. size(u) over the composite grid along axis (1-based): out(bin, row) -- row r of vdn_profile_layout's
  ! 0-based count is out(:, r + 1) -- and cells(bin), both of profiles_nbins bins.  No ghost cell is read
  subroutine profiles(mla, u, s, dx, axis, out, cells)
    type(ml_layout), intent(in   ) :: mla
    type(multifab) , intent(in   ) :: u(:), s(:)
    real(dp_t)     , intent(in   ) :: dx(:,:)
    integer        , intent(in   ) :: axis
    real(dp_t)     , intent(  out) :: out(:,:)
    integer(c_long_long), intent(out) :: cells(:)
    real(c_double) :: dxc(3 * size(u))
    real(c_double), allocatable :: o(:)
    integer(c_long_long), allocatable :: cc(:)
    integer :: n, d, nb, nr
    nb = profiles_nbins(mla, size(u), axis)
    nr = size(out, 2)
    if (size(out, 1) /= nb .or. size(cells) /= nb) error stop 'profiles: out(nbins, nrow) and cells(nbins) with nbins = profiles_nbins expected'
    dxc = 1.0_c_double
    do n = 1, size(u)
       do d = 1, min(3, size(dx, 2))
          dxc((n - 1) * 3 + d) = dx(n, d)
       end do
    end do
    allocate(o(nb * nr), cc(nb))
    call chk(vdn_profiles(int(size(u), c_int), mla%h, handles(u), handles(s), dxc, int(axis - 1, c_int), int(nb, c_long), o, cc), 'profiles')
    out = reshape(o, (/ nb, nr /))
    cells = cc
  end subroutine profiles
  subroutine make_magvel(magvel, comp, u)
    type(multifab), intent(inout) :: magvel, u
    integer       , intent(in   ) :: comp
    call chk(vdn_make_magvel(magvel%h, int(comp - 1, c_int), u%h), 'make_magvel')
  end subroutine make_magvel
  subroutine ml_nodal_prolongation(fine, crse)
    type(multifab), intent(inout) :: fine, crse
    call chk(vdn_ml_nodal_prolongation(fine%h, crse%h), 'ml_nodal_prolongation')
  end subroutine ml_nodal_prolongation
  subroutine multifab_copy_layouts(dst, dcomp, src, scomp, nc)
    type(multifab), intent(inout) :: dst
    type(multifab), intent(in   ) :: src
    integer       , intent(in   ) :: dcomp, scomp, nc
    call chk(vdn_multifab_copy_layouts(dst%h, int(dcomp - 1, c_int), src%h, int(scomp - 1, c_int), int(nc, c_int)), 'multifab_copy_c')
  end subroutine multifab_copy_layouts
  ! tag_boxes + make_new_grids (src/initialize.f90:247-248, src/regrid.f90:148-149): the boxes of level lev+1 from the state of level lev
  subroutine make_new_grids(new_grid, mf, lev, buf_wid, nest, max_grid_size, boxes, nboxes)
    logical       , intent(  out) :: new_grid
    type(multifab), intent(in   ) :: mf
    integer       , intent(in   ) :: lev, buf_wid, nest, max_grid_size
    type(vdn_box) , intent(  out) :: boxes(:)
    integer       , intent(  out) :: nboxes
    integer(c_int)  :: nb
    integer(c_long) :: nt
    call chk(vdn_make_new_grids(mf%h, int(lev, c_int), int(buf_wid, c_int), int(nest, c_int), 0.9_c_double, 4_c_int, 4_c_int, &
                                int(max_grid_size, c_int), int(size(boxes), c_int), boxes, nb, nt), 'make_new_grids')
    nboxes = nb
    new_grid = nb > 0
  end subroutine make_new_grids
  ! the same with the cells tagged by criteria chosen at run time instead of the rules of src/tag_boxes.f90 (the stand-in for editing that file): crit(1:ncrit) as
  ! make_tag_criterion builds them; u, dx and the_bc_tower are read by the velocity criteria (the call fills the ghost cells of u as make_vorticity does)
  subroutine make_new_grids_by(new_grid, mf, u, dx, the_bc_tower, lev, ncrit, crit, buf_wid, nest, max_grid_size, boxes, nboxes)
    logical       , intent(  out) :: new_grid
    type(multifab), intent(in   ) :: mf
    type(multifab), intent(inout) :: u
    real(dp_t)    , intent(in   ) :: dx(:)
    type(bc_tower), intent(in   ) :: the_bc_tower
    integer       , intent(in   ) :: lev, ncrit, buf_wid, nest, max_grid_size
    type(vdn_tag_criterion), intent(in) :: crit(:)
    type(vdn_box) , intent(  out) :: boxes(:)
    integer       , intent(  out) :: nboxes
    integer(c_int)  :: nb
    integer(c_long) :: nt
    real(c_double)  :: d(3)
    d = 1.0_c_double; d(1:min(3, size(dx))) = dx(1:min(3, size(dx)))
    call chk(vdn_make_new_grids_by(mf%h, u%h, d, the_bc_tower%h, int(lev, c_int), int(ncrit, c_int), crit, int(buf_wid, c_int), int(nest, c_int), &
                                   0.9_c_double, 4_c_int, 4_c_int, int(max_grid_size, c_int), int(size(boxes), c_int), boxes, nb, nt), 'make_new_grids_by')
    nboxes = nb
    new_grid = nb > 0
  end subroutine make_new_grids_by
  ! the tag bitmap of the criteria alone: one byte per cell of the level's domain, x fastest
  subroutine tag_boxes_by(tags, mf, u, dx, the_bc_tower, lev, ncrit, crit)
    integer(c_signed_char), intent(out) :: tags(*)
    type(multifab), intent(in   ) :: mf
    type(multifab), intent(inout) :: u
    real(dp_t)    , intent(in   ) :: dx(:)
    type(bc_tower), intent(in   ) :: the_bc_tower
    integer       , intent(in   ) :: lev, ncrit
    type(vdn_tag_criterion), intent(in) :: crit(:)
    real(c_double)  :: d(3)
    d = 1.0_c_double; d(1:min(3, size(dx))) = dx(1:min(3, size(dx)))
    call chk(vdn_tag_boxes_by(mf%h, u%h, d, the_bc_tower%h, int(lev, c_int), int(ncrit, c_int), crit, tags), 'tag_boxes_by')
  end subroutine tag_boxes_by
  ! one criterion from the namelist's form: the field by name, comp 1-based, the thresholds of levels 1 .. 4 with `unset` where the inputs gave none -- an unset
  ! level repeats the level before it (the reference's "case default"), a side never set is open
  function make_tag_criterion(field, comp, gt, lt, unset) result(c)
    use, intrinsic :: ieee_arithmetic, only: ieee_value, ieee_negative_inf, ieee_positive_inf
    character(len=*), intent(in) :: field
    integer         , intent(in) :: comp
    real(dp_t)      , intent(in) :: gt(4), lt(4), unset
    type(vdn_tag_criterion) :: c
    integer :: l
    select case (trim(field))
    case ('scalar');      c%field = VDN_TAG_SCALAR
    case ('scalar_grad'); c%field = VDN_TAG_SCALAR_GRAD
    case ('vorticity');   c%field = VDN_TAG_VORTICITY
    case ('magvel');      c%field = VDN_TAG_MAGVEL
    case default
       write(*, '(a,a)') 'varden_amd: unknown tag_field ', trim(field)
       error stop 1
    end select
    c%comp = comp - 1
    c%gt = ieee_value(1.0_c_double, ieee_negative_inf); c%lt = ieee_value(1.0_c_double, ieee_positive_inf)      ! open sides
    do l = 1, 4
       if (gt(l) /= unset) then
          c%gt(l) = gt(l)
       else if (l > 1) then
          c%gt(l) = c%gt(l - 1)
       end if
       if (lt(l) /= unset) then
          c%lt(l) = lt(l)
       else if (l > 1) then
          c%lt(l) = c%lt(l - 1)
       end if
    end do
  end function make_tag_criterion

  ! ---- plot files and checkpoints (FBoxLib's fabio_module, src/checkpoint.f90): written and read inside the library, one rank ------------------------
  ! fabio_ml_multifab_write_d(mfs, rrs, dirname, names, bounding_box, prob_lo, prob_hi, time, dx)   (src/varden.f90:568-573, src/checkpoint.f90:45-48);
  ! rr: one ratio per pair of levels; the optional arguments default as in fabio (names Var-i, the bounding box of level 1, the unit mesh)
  subroutine fabio_ml_multifab_write_d(mfs, rr, dirname, names, bounding_box, prob_lo, prob_hi, time, dx, staging_bytes)
    type(multifab)  , intent(in) :: mfs(:)
    integer         , intent(in) :: rr(:)
    character(len=*), intent(in) :: dirname
    character(len=*), intent(in), optional :: names(:)
    type(vdn_box)   , intent(in), optional :: bounding_box
    real(dp_t)      , intent(in), optional :: prob_lo(:), prob_hi(:), time, dx(:)
    integer(c_long) , intent(in), optional :: staging_bytes
    call fabio_write_any(mfs, rr, dirname, names, bounding_box, prob_lo, prob_hi, time, dx, staging_bytes)
  end subroutine fabio_ml_multifab_write_d
  ! plane k = 0 of the 3-D multifabs of a z-uniform copy as a dm = 2 hierarchy: file component c = component comps(c) (1-based); bounding_box, prob_lo, prob_hi
  ! and dx give their two in-plane entries.  defect: largest |f(i,j,k) - f(i,j,0)| over the listed components, largest |value| of the components vanish(:)
  subroutine fabio_ml_multifab_write_plane_d(mfs, rr, dirname, comps, names, bounding_box, prob_lo, prob_hi, time, dx, staging_bytes, vanish, defect)
    type(multifab)  , intent(in) :: mfs(:)
    integer         , intent(in) :: rr(:), comps(:)
    character(len=*), intent(in) :: dirname
    character(len=*), intent(in), optional :: names(:)
    type(vdn_box)   , intent(in), optional :: bounding_box
    real(dp_t)      , intent(in), optional :: prob_lo(:), prob_hi(:), time, dx(:)
    integer(c_long) , intent(in), optional :: staging_bytes
    integer         , intent(in), optional :: vanish(:)
    real(dp_t)      , intent(out), optional :: defect(2)
    call fabio_write_any(mfs, rr, dirname, names, bounding_box, prob_lo, prob_hi, time, dx, staging_bytes, comps, vanish, defect)
  end subroutine fabio_ml_multifab_write_plane_d
  subroutine fabio_write_any(mfs, rr, dirname, names, bounding_box, prob_lo, prob_hi, time, dx, staging_bytes, comps, vanish, defect)
    type(multifab)  , intent(in) :: mfs(:)
    integer         , intent(in) :: rr(:)
    character(len=*), intent(in) :: dirname
    character(len=*), intent(in), optional :: names(:)
    type(vdn_box)   , intent(in), optional :: bounding_box
    real(dp_t)      , intent(in), optional :: prob_lo(:), prob_hi(:), time, dx(:)
    integer(c_long) , intent(in), optional :: staging_bytes
    integer         , intent(in), optional :: comps(:), vanish(:)
    real(dp_t)      , intent(out), optional :: defect(2)
    integer(c_int), allocatable :: cc(:), vc(:)
    real(c_double), target :: dfc(2)
    type(c_ptr) :: a_def
    integer :: nv
    character(kind=c_char), allocatable, target :: cbuf(:,:)
    type(c_ptr), allocatable, target :: cp(:)
    type(vdn_box), target :: pd
    real(c_double), target :: plo(3), phi(3), dxc(3)
    real(c_double) :: t
    integer(c_int) :: rrc(max(1, size(rr)))
    integer(c_long) :: sb
    type(c_ptr) :: a_names, a_pd, a_lo, a_hi, a_dx
    integer :: i, j, n
    rrc = 2; rrc(1:size(rr)) = rr
    a_names = c_null_ptr; a_pd = c_null_ptr; a_lo = c_null_ptr; a_hi = c_null_ptr; a_dx = c_null_ptr
    if (present(names)) then
       allocate(cbuf(len(names) + 1, size(names)), cp(size(names)))
       do i = 1, size(names)
          n = len_trim(names(i))
          do j = 1, n
             cbuf(j, i) = names(i)(j:j)
          end do
          cbuf(n + 1, i) = c_null_char
          cp(i) = c_loc(cbuf(1, i))
       end do
       a_names = c_loc(cp(1))
    end if
    if (present(bounding_box)) then
       pd = bounding_box; a_pd = c_loc(pd)
    end if
    plo = 0.d0; phi = 1.d0; dxc = 1.d0
    if (present(prob_lo)) then
       plo(1:size(prob_lo)) = prob_lo; a_lo = c_loc(plo(1))
    end if
    if (present(prob_hi)) then
       phi(1:size(prob_hi)) = prob_hi; a_hi = c_loc(phi(1))
    end if
    if (present(dx)) then
       dxc(1:size(dx)) = dx; a_dx = c_loc(dxc(1))
    end if
    t = 0.d0; if (present(time)) t = time
    sb = 0; if (present(staging_bytes)) sb = staging_bytes
    if (.not. present(comps)) then
       call chk(vdn_fabio_ml_multifab_write_d(trim(dirname) // c_null_char, int(size(mfs), c_int), handles(mfs), rrc, a_names, a_pd, a_lo, a_hi, t, a_dx, sb), &
                'fabio_ml_multifab_write_d')
       return
    end if
    allocate(cc(size(comps))); cc = int(comps - 1, c_int)
    nv = 0; if (present(vanish)) nv = size(vanish)
    allocate(vc(max(1, nv))); vc = 0
    if (nv > 0) vc(1:nv) = int(vanish - 1, c_int)
    a_def = c_null_ptr; if (present(defect)) a_def = c_loc(dfc(1))
    call chk(vdn_fabio_ml_multifab_write_plane_d(trim(dirname) // c_null_char, int(size(mfs), c_int), handles(mfs), rrc, a_names, a_pd, a_lo, a_hi, t, a_dx, sb, &
                                                 int(size(comps), c_int), cc, int(nv, c_int), vc, a_def), &
             'fabio_ml_multifab_write_plane_d')
    if (present(defect)) defect = dfc
  end subroutine fabio_write_any

  ! what fabio_ml_multifab_read_d learns from the files before it builds its layout (text only: needs no GPU); nboxes(:) and rr(:) hold 4 entries at least
  subroutine fabio_ml_multifab_info(dirname, nlev, dm, ncomp, nodal, nboxes, rr, time)
    character(len=*), intent(in) :: dirname
    integer, intent(out) :: nlev, dm, ncomp, nboxes(:), rr(:)
    logical, intent(out) :: nodal(3)
    real(dp_t), intent(out) :: time
    integer(c_int) :: nl, d, nc, nd(3), nb(4), r(4)
    nb = 0; r = 2
    call chk(vdn_fabio_ml_multifab_info(trim(dirname) // c_null_char, nl, d, nc, nd, nb, r, time), 'fabio_ml_multifab_info')
    nlev = nl; dm = d; ncomp = nc; nodal = nd /= 0
    nboxes = 0; nboxes(1:nl) = nb(1:nl)
    rr = 2; if (nl > 1) rr(1:nl - 1) = r(1:nl - 1)
  end subroutine fabio_ml_multifab_info

  ! the cell boxes of level lev (1-based) of a hierarchy on disk, in the file's order
  subroutine fabio_ml_multifab_boxes(dirname, lev, boxes)
    character(len=*), intent(in) :: dirname
    integer, intent(in) :: lev
    type(vdn_box), intent(out) :: boxes(:)
    call chk(vdn_fabio_ml_multifab_boxes(trim(dirname) // c_null_char, int(lev - 1, c_int), boxes, int(size(boxes), c_int)), 'fabio_ml_multifab_boxes')
  end subroutine fabio_ml_multifab_boxes

  ! the data of fabio_ml_multifab_read_d (src/checkpoint.f90:130,134) into multifabs built on the file's box lists: valid points only
  subroutine fabio_ml_multifab_read_d(mfs, dirname, staging_bytes)
    type(multifab)  , intent(inout) :: mfs(:)
    character(len=*), intent(in) :: dirname
    integer(c_long) , intent(in), optional :: staging_bytes
    integer(c_long) :: sb
    sb = 0; if (present(staging_bytes)) sb = staging_bytes
    call chk(vdn_fabio_ml_multifab_read_d(trim(dirname) // c_null_char, int(size(mfs), c_int), handles(mfs), sb), 'fabio_ml_multifab_read_d')
  end subroutine fabio_ml_multifab_read_d

  ! a dm = 2 hierarchy on disk into the 3-D multifabs of a copy (cut along z in any way): file component c to every valid z-plane of comps(c) (1-based)
  subroutine fabio_ml_multifab_read_plane_d(mfs, dirname, comps, staging_bytes)
    type(multifab)  , intent(inout) :: mfs(:)
    character(len=*), intent(in) :: dirname
    integer         , intent(in) :: comps(:)
    integer(c_long) , intent(in), optional :: staging_bytes
    integer(c_long) :: sb
    integer(c_int) :: cc(size(comps))
    sb = 0; if (present(staging_bytes)) sb = staging_bytes
    cc = int(comps - 1, c_int)
    call chk(vdn_fabio_ml_multifab_read_plane_d(trim(dirname) // c_null_char, int(size(mfs), c_int), handles(mfs), sb, int(size(comps), c_int), cc), &
             'fabio_ml_multifab_read_plane_d')
  end subroutine fabio_ml_multifab_read_plane_d

  ! checkpoint_write of a z-uniform copy: State = the components comps(:) of mfs, Pressure = mfs_nodal (nodal (1,1) in the file); defect as above
  subroutine checkpoint_write_plane(dirname, mfs, mfs_nodal, rr, time, dt, comps, vanish, defect)
    character(len=*), intent(in) :: dirname
    type(multifab)  , intent(in) :: mfs(:), mfs_nodal(:)
    integer         , intent(in) :: rr(:), comps(:), vanish(:)
    real(dp_t)      , intent(in) :: time, dt
    real(dp_t)      , intent(out) :: defect(2)
    integer(c_int) :: rrc(max(1, size(rr))), cc(size(comps)), vc(max(1, size(vanish)))
    rrc = 2; rrc(1:size(rr)) = rr
    cc = int(comps - 1, c_int); vc = 0; vc(1:size(vanish)) = int(vanish - 1, c_int)
    call chk(vdn_checkpoint_write_plane(trim(dirname) // c_null_char, int(size(mfs), c_int), handles(mfs), handles(mfs_nodal), rrc, time, dt, 0_c_long, &
                                        int(size(comps), c_int), cc, int(size(vanish), c_int), vc, defect), 'checkpoint_write_plane')
  end subroutine checkpoint_write_plane

  ! checkpoint_write(nlevs, dirname, mfs, mfs_nodal, rrs, time, dt)   (src/checkpoint.f90:14-83): State, Pressure and the Header namelist
  subroutine checkpoint_write(dirname, mfs, mfs_nodal, rr, time, dt)
    character(len=*), intent(in) :: dirname
    type(multifab)  , intent(in) :: mfs(:), mfs_nodal(:)
    integer         , intent(in) :: rr(:)
    real(dp_t)      , intent(in) :: time, dt
    integer(c_int) :: rrc(max(1, size(rr)))
    rrc = 2; rrc(1:size(rr)) = rr
    call chk(vdn_checkpoint_write(trim(dirname) // c_null_char, int(size(mfs), c_int), handles(mfs), handles(mfs_nodal), rrc, time, dt, 0_c_long), &
             'checkpoint_write')
  end subroutine checkpoint_write

  ! the Header of checkpoint_read (src/checkpoint.f90:112-126): nlevs, time, dt and the ratios (rr(:) holds 4 entries at least)
  subroutine checkpoint_info(dirname, nlev, time, dt, rr)
    character(len=*), intent(in) :: dirname
    integer, intent(out) :: nlev, rr(:)
    real(dp_t), intent(out) :: time, dt
    integer(c_int) :: nl, r(4)
    r = 2
    call chk(vdn_checkpoint_info(trim(dirname) // c_null_char, nl, time, dt, r), 'checkpoint_info')
    nlev = nl
    rr = 2; if (nl > 1) rr(1:nl - 1) = r(1:nl - 1)
  end subroutine checkpoint_info

  ! ---- values at points and tracer particles: the definitions are stated with the C entries in include/varden_amd.h.  Components are 1-based here; positions are
  ! x(3, n), values val(nc, n), columns cols(n, ncol) ----------------------------------------------------------------------------------------------------------
  function dx_levels(dx, nlev) result(dxc)
    real(dp_t), intent(in) :: dx(:,:)
    integer, intent(in) :: nlev
    real(c_double) :: dxc(3 * nlev)
    integer :: n, d
    dxc = 1.0_c_double
    do n = 1, nlev
       do d = 1, min(3, size(dx, 2))
          dxc((n - 1) * 3 + d) = dx(n, d)
       end do
    end do
  end function dx_levels

  subroutine sample_points(mla, mf, comp, nc, bccomp, dx, the_bc_tower, x, val, lev)
    type(ml_layout), intent(in   ) :: mla
    type(multifab) , intent(in   ) :: mf(:)
    integer        , intent(in   ) :: comp, nc, bccomp
    real(dp_t)     , intent(in   ) :: dx(:,:), x(:,:)
    type(bc_tower) , intent(in   ) :: the_bc_tower
    real(dp_t)     , intent(  out) :: val(:,:)
    integer        , intent(  out) :: lev(:)
    integer(c_int) :: levc(size(x, 2))
    call chk(vdn_sample_points(int(size(mf), c_int), mla%h, handles(mf), int(comp - 1, c_int), int(nc, c_int), int(bccomp - 1, c_int), dx_levels(dx, size(mf)), &
                               the_bc_tower%h, int(size(x, 2), c_long), x, val, levc), 'sample_points')
    lev = levc
  end subroutine sample_points

  ! the surface mf(comp) = value over the composite grid of levels 1 .. size(mf) (see vdn_isosurface): counts, area, area vector and volumes in iso; with tri and
  ! lev also the triangles, tri(direction, vertex, triangle) in output order, and their levels (numbered from 0, as the library numbers them) -- the call sizes
  ! itself: a count call first, then the triangles.  comp and bccomp are numbered from 1; the CALLER has filled the ghost cells of mf; dm = 3 only
  subroutine isosurface(mla, mf, comp, bccomp, dx, the_bc_tower, value, iso, tri, lev)
    type(ml_layout), intent(in   ) :: mla
    type(multifab) , intent(in   ) :: mf(:)
    integer        , intent(in   ) :: comp, bccomp
    real(dp_t)     , intent(in   ) :: dx(:,:), value
    type(bc_tower) , intent(in   ) :: the_bc_tower
    type(vdn_iso)  , intent(  out) :: iso
    real(dp_t)        , allocatable, target, intent(out), optional :: tri(:,:,:)
    integer(c_int8_t), allocatable, target, intent(out), optional :: lev(:)
    integer(c_long_long) :: n
    if (vdn_iso_sizeof() /= c_sizeof(iso)) error stop 'isosurface: vdn_iso differs between the library and this module'
    if (present(tri) .neqv. present(lev)) error stop 'isosurface: tri and lev come together'
    call chk(vdn_isosurface(int(size(mf), c_int), mla%h, handles(mf), int(comp - 1, c_int), int(bccomp - 1, c_int), dx_levels(dx, size(mf)), the_bc_tower%h, &
                            value, 0_c_long_long, c_null_ptr, c_null_ptr, iso), 'isosurface')
    if (.not. present(tri)) return
    n = iso%ntri
    allocate(tri(3, 3, n), lev(n))
    if (n == 0) return
    call chk(vdn_isosurface(int(size(mf), c_int), mla%h, handles(mf), int(comp - 1, c_int), int(bccomp - 1, c_int), dx_levels(dx, size(mf)), the_bc_tower%h, &
                            value, n, c_loc(tri), c_loc(lev), iso), 'isosurface')
    if (iso%written /= n) error stop 'isosurface: the triangles counted were not written'
  end subroutine isosurface

  ! the triangles of isosurface as binary PLY (see vdn_isosurface_write); rank 0 writes
  subroutine isosurface_write(path, tri, lev, value, time)
    character(len=*) , intent(in) :: path
    real(dp_t)       , intent(in), target, contiguous :: tri(:,:,:)
    integer(c_int8_t), intent(in), target, contiguous :: lev(:)
    real(dp_t)       , intent(in) :: value, time
    if (size(tri, 1) /= 3 .or. size(tri, 2) /= 3 .or. size(tri, 3) /= size(lev)) error stop 'isosurface_write: tri(3, 3, ntri) and lev(ntri) expected'
    if (size(lev) == 0) then
       call chk(vdn_isosurface_write(trim(path) // c_null_char, 0_c_long_long, c_null_ptr, c_null_ptr, value, time), 'isosurface_write')
    else
       call chk(vdn_isosurface_write(trim(path) // c_null_char, int(size(lev), c_long_long), c_loc(tri), c_loc(lev), value, time), 'isosurface_write')
    end if
  end subroutine isosurface_write

  subroutine particles_create(p, x)
    type(particles), intent(  out) :: p
    real(dp_t)     , intent(in   ) :: x(:,:)
    call chk(vdn_particles_create(int(size(x, 2), c_long), x, p%h), 'particles_create')
    p%n = size(x, 2)
  end subroutine particles_create

  subroutine particles_destroy(p)
    type(particles), intent(inout) :: p
    call chk(vdn_particles_destroy(p%h), 'particles_destroy')
    p%h = c_null_ptr; p%n = 0
  end subroutine particles_destroy

  function particles_count(p) result(active)
    type(particles), intent(in) :: p
    integer :: active
    integer(c_long) :: n, a
    call chk(vdn_particles_count(p%h, n, a), 'particles_count')
    active = int(a)
  end function particles_count

  subroutine particles_get(p, x, state)
    type(particles), intent(in   ) :: p
    real(dp_t)     , intent(  out) :: x(:,:)
    integer        , intent(  out) :: state(:)
    integer(c_int) :: st(p%n)
    call chk(vdn_particles_get(p%h, x, st), 'particles_get')
    state = st
  end subroutine particles_get

  ! one move from the velocity u0 (old time) to u1 (new time), both with their ghost cells filled
  subroutine particles_advance(p, mla, u0, u1, dx, the_bc_tower, dt)
    type(particles), intent(inout) :: p
    type(ml_layout), intent(in   ) :: mla
    type(multifab) , intent(in   ) :: u0(:), u1(:)
    real(dp_t)     , intent(in   ) :: dx(:,:), dt
    type(bc_tower) , intent(in   ) :: the_bc_tower
    call chk(vdn_particles_advance(p%h, int(size(u0), c_int), mla%h, handles(u0), handles(u1), dx_levels(dx, size(u0)), the_bc_tower%h, dt), 'particles_advance')
  end subroutine particles_advance

  subroutine particles_sample(p, mla, mf, comp, nc, bccomp, dx, the_bc_tower, val, lev)
    type(particles), intent(in   ) :: p
    type(ml_layout), intent(in   ) :: mla
    type(multifab) , intent(in   ) :: mf(:)
    integer        , intent(in   ) :: comp, nc, bccomp
    real(dp_t)     , intent(in   ) :: dx(:,:)
    type(bc_tower) , intent(in   ) :: the_bc_tower
    real(dp_t)     , intent(  out) :: val(:,:)
    integer        , intent(  out) :: lev(:)
    integer(c_int) :: levc(p%n)
    call chk(vdn_particles_sample(p%h, int(size(mf), c_int), mla%h, handles(mf), int(comp - 1, c_int), int(nc, c_int), int(bccomp - 1, c_int), &
                                  dx_levels(dx, size(mf)), the_bc_tower%h, val, levc), 'particles_sample')
    lev = levc
  end subroutine particles_sample

  ! one particle file: header, states, positions and the columns cols(n, ncol) under names(ncol) (one word each, 64 characters at the most)
  subroutine particles_write(p, path, time, names, cols)
    type(particles) , intent(in) :: p
    character(len=*), intent(in) :: path, names(:)
    real(dp_t)      , intent(in) :: time, cols(:,:)
    character(kind=c_char), target :: cbuf(65, max(1, size(names)))
    type(c_ptr) :: ptrs(max(1, size(names)))
    integer :: i, j, n
    do i = 1, size(names)
       n = min(64, len_trim(names(i)))
       do j = 1, n
          cbuf(j, i) = names(i)(j:j)
       end do
       cbuf(n + 1, i) = c_null_char
       ptrs(i) = c_loc(cbuf(1, i))
    end do
    call chk(vdn_particles_write(p%h, trim(path) // c_null_char, time, int(size(names), c_int), ptrs, cols), 'particles_write')
  end subroutine particles_write

  subroutine particles_read(path, p, time)
    character(len=*), intent(in   ) :: path
    type(particles) , intent(  out) :: p
    real(dp_t)      , intent(  out) :: time
    integer(c_long) :: n, a
    call chk(vdn_particles_read(trim(path) // c_null_char, p%h, time), 'particles_read')
    call chk(vdn_particles_count(p%h, n, a), 'particles_read')
    p%n = int(n)
  end subroutine particles_read

  function handles(mfs) result(h)
    type(multifab), intent(in) :: mfs(:)
    type(c_ptr) :: h(size(mfs))
    integer :: n
    do n = 1, size(mfs)
       h(n) = mfs(n)%h
    end do
  end function handles

end module varden_amd
