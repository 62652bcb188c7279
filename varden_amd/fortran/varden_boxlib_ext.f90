! varden_boxlib_ext.f90 -- FBoxLib / VARDEN modules BEYOND the hot path's own that the reference's callers `use` and that are thin over the C-ABI.
!
! tools/check_reference_callers.py runs `flang -fsyntax-only` on the reference's own callers of the hot path (src/varden.f90, src/advance_timestep.f90,
! src/initialize.f90, src/regrid.f90, ... read IN PLACE from the reference tree, nothing copied) against the modules of varden_boxlib.f90 and of this
! file, and lists what is still missing (profiles/r06_reference_callers_syntax.txt; INTEGRATION.md section 2 reads it).  The modules here:
!   parallel            parallel_myproc / nprocs / IOProcessor / IOProcessorNode / wtime / barrier / reduce (MPI_MAX, MPI_MIN, MPI_SUM), one rank per GPU:
!                       the ranks of varden_amd_initialize; reductions across ranks go through vdn_comm_allreduce_max (RCCL)
!   BoxLib              boxlib_initialize / boxlib_finalize (src/main.f90:8,17): rank and device from the launcher's environment (RANK / LOCAL_RANK /
!                       WORLD_SIZE as torchrun and bench.py export them, else one rank)
!   bl_error_module     bl_error / bl_warn / bl_assert
!   bl_prof_module      type bl_prof_timer, build(bpt, name) / destroy(bpt) (src/advance_timestep.f90:58-60,99-101): the library opens the roctx ranges of
!                       these names itself (runtime.hip: Prof), so the host-side timers are empty here
!   bl_IO_module        unit_new
!   vort_module         make_vorticity(vort, comp, u, dx, bc) / make_magvel(magvel, comp, u)   (src/makevort.f90:16,58)
!   fillpatch_module, ml_prolongation_module   fillpatch(fine, crse, ...) / ml_nodal_prolongation(fine, crse, ir)   (src/regrid.f90:279-280, 317-344)
!   fabio_module        fabio_mkdir / fabio_ml_multifab_write_d(mfs, rrs, dirname[, names, bounding_box, prob_lo, prob_hi, time, dx]) / fabio_ml_multifab_read_d(mfs,
!                       dirname)   (src/varden.f90:568-573, src/checkpoint.f90:40-48, 130-134): the library packs and writes (csrc/fabio.hip); one rank
!   profiles_module     profiles_layout / profiles_nbins(mla, axis) / profiles(mla, u, s, dx, axis, out, cells): the plane-averaged profiles of varden_amd on these
!                       container types (the project's own analysis call; the reference has none)
! probin_module (varden_boxlib.f90) carries every entry of src/_parameters with its default, the &PROBIN namelist, probin_init and probin_close.
! NOT here (listed by the report as the maintainer's remaining work): FBoxLib's host-side box calculus (list_box_module, box_util_module), plotfile_module,
! bl_timer, layouts built one level at a time (layout_build_ba, make_new_grids_module, tag_boxes_module --
! the library builds whole hierarchies: vdn_make_new_grids), and the modules INSIDE advance_timestep (pre_advance_module, scalar_advance_module, ...): the
! boundary is advance_timestep itself, their kernels are the vdn_k_* hooks of include/varden_amd.h.

module BoxLib
  use parallel
  use bl_error_module
  implicit none
contains
  ! src/main.f90:8: one rank per GPU; the rank, the world size and the device come from the launcher (torchrun / bench.py / mpirun export one of these sets)
  subroutine boxlib_initialize()
    integer :: rank, nranks
    rank = env_int('RANK', env_int('OMPI_COMM_WORLD_RANK', 0))
    nranks = env_int('WORLD_SIZE', env_int('OMPI_COMM_WORLD_SIZE', 1))
    call parallel_set_ranks(rank, nranks)
  end subroutine boxlib_initialize
  subroutine boxlib_finalize()
  end subroutine boxlib_finalize
  integer function boxlib_device()
    boxlib_device = env_int('LOCAL_RANK', env_int('OMPI_COMM_WORLD_LOCAL_RANK', 0))
  end function boxlib_device
  integer function env_int(name, dflt)
    character(len=*), intent(in) :: name
    integer, intent(in) :: dflt
    character(len=32) :: v
    integer :: st, ios
    env_int = dflt
    call get_environment_variable(name, v, status=st)
    if (st /= 0) return
    read(v, *, iostat=ios) env_int
    if (ios /= 0) env_int = dflt
  end function env_int
end module BoxLib

module vort_module
  use multifab_module
  use define_bc_module
  use varden_amd, only: vamd_make_vorticity => make_vorticity, vamd_make_magvel => make_magvel
  implicit none
contains
  ! make_vorticity(vort, comp, u, dx, bc)   (src/makevort.f90:16-22)
  subroutine make_vorticity(vort, comp, u, dx, bc)
    integer, intent(in) :: comp
    type(multifab), intent(inout) :: vort
    type(multifab), intent(inout) :: u
    real(dp_t), intent(in) :: dx(:)
    type(bc_level), intent(in) :: bc
    call vamd_make_vorticity(vort%v, comp, u%v, dx, as_vamd_tower(bc))
  end subroutine make_vorticity
  ! make_magvel(magvel, comp, u)   (src/makevort.f90:58-62)
  subroutine make_magvel(magvel, comp, u)
    integer, intent(in) :: comp
    type(multifab), intent(inout) :: magvel
    type(multifab), intent(inout) :: u
    call vamd_make_magvel(magvel%v, comp, u%v)
  end subroutine make_magvel
end module vort_module

module fillpatch_module
  use multifab_module
  use define_bc_module
  use varden_amd, only: vamd_fillpatch => fillpatch
  implicit none
contains
  ! fillpatch(fine, crse, ng, ir, bc_crse, bc_fine, icomp_fine, icomp_crse, bcomp, nc)   (FBoxLib; src/regrid.f90:317-330): every point of the new fine level
  ! from the coarse level (the caller then copies the old fine data over it).  The coarse and fine components coincide at every call site of the reference.
  subroutine fillpatch(fine, crse, ng, ir, bc_crse, bc_fine, icomp_fine, icomp_crse, bcomp, nc, no_final_physbc_input, lim_slope_input, lin_limit_input, &
                       fill_crse_input, stencil_width_input, fourth_order_input)
    type(multifab), intent(inout) :: fine, crse
    integer, intent(in) :: ng, ir(:), icomp_fine, icomp_crse, bcomp, nc
    type(bc_level), intent(in) :: bc_crse, bc_fine
    ! FBoxLib's options; the reference passes no_final_physbc_input = .true. only (the library's fillpatch applies no physical boundary: the caller does)
    logical, intent(in), optional :: no_final_physbc_input, lim_slope_input, lin_limit_input, fill_crse_input, fourth_order_input
    integer, intent(in), optional :: stencil_width_input
    if (any(ir /= 2)) error stop 'fillpatch: refinement ratio 2 only'
    if (icomp_fine /= icomp_crse) error stop 'fillpatch: the coarse and fine components must coincide'
    call vamd_fillpatch(fine%v, crse%v, icomp_fine, nc)
  end subroutine fillpatch
end module fillpatch_module

module ml_prolongation_module
  use multifab_module
  use varden_amd, only: vamd_nodal_prolongation => ml_nodal_prolongation
  implicit none
contains
  ! ml_nodal_prolongation(fine, crse, ir)   (FBoxLib; src/regrid.f90:342-344: the pressure of a new fine level)
  subroutine ml_nodal_prolongation(fine, crse, ir)
    type(multifab), intent(inout) :: fine, crse
    integer, intent(in) :: ir(:)
    if (any(ir /= 2)) error stop 'ml_nodal_prolongation: refinement ratio 2 only'
    call vamd_nodal_prolongation(fine%v, crse%v)
  end subroutine ml_nodal_prolongation
end module ml_prolongation_module

module fabio_module
  use iso_c_binding
  use bl_types
  use box_module
  use ml_boxarray_module
  use ml_layout_module
  use multifab_module
  use varden_amd, only: vamd_multifab => multifab, vamd_write_d => fabio_ml_multifab_write_d, vamd_info => fabio_ml_multifab_info, &
                        vamd_boxes => fabio_ml_multifab_boxes, vamd_read_d => fabio_ml_multifab_read_d, vdn_box
  implicit none
  private
  public :: fabio_mkdir, fabio_ml_multifab_write_d, fabio_ml_multifab_read_d
  ! the hierarchies fabio_ml_multifab_read_d built its multifabs on: they live as long as the program (FBoxLib's read leaves its layouts to the caller's multifabs)
  type(ml_layout), save, target :: read_mla(16)
  integer, save :: nread = 0
  interface
     integer(c_int) function c_mkdir(path, mode) bind(C, name="mkdir")
       import :: c_int, c_char
       character(kind=c_char), intent(in) :: path(*)
       integer(c_int), value :: mode
     end function c_mkdir
  end interface
contains
  ! fabio_mkdir(dirname)   (src/checkpoint.f90:40); an existing directory is kept
  subroutine fabio_mkdir(dirname, stat)
    character(len=*), intent(in) :: dirname
    integer, intent(out), optional :: stat
    integer(c_int) :: rc
    rc = c_mkdir(trim(dirname) // c_null_char, int(o'777', c_int))
    if (present(stat)) stat = 0
  end subroutine fabio_mkdir

  ! fabio_ml_multifab_write_d(mfs, rrs, dirname, names, bounding_box, prob_lo, prob_hi, time, dx)   (src/varden.f90:572, src/checkpoint.f90:45)
  subroutine fabio_ml_multifab_write_d(mfs, rrs, dirname, names, bounding_box, prob_lo, prob_hi, time, dx)
    type(multifab)  , intent(in) :: mfs(:)
    integer         , intent(in) :: rrs(:)
    character(len=*), intent(in) :: dirname
    character(len=*), intent(in), optional :: names(:)
    type(box)       , intent(in), optional :: bounding_box
    real(dp_t)      , intent(in), optional :: prob_lo(:), prob_hi(:), time, dx(:)
    type(vamd_multifab) :: v(size(mfs))
    type(vdn_box) :: pd
    integer :: n, nr
    do n = 1, size(mfs)
       v(n) = mfs(n)%v
    end do
    nr = min(size(rrs), size(mfs) - 1)
    if (present(bounding_box)) then
       pd%lo = 0; pd%hi = 0
       pd%lo(1:bounding_box%dim) = bounding_box%lo(1:bounding_box%dim); pd%hi(1:bounding_box%dim) = bounding_box%hi(1:bounding_box%dim)
       call vamd_write_d(v, rrs(1:nr), dirname, names, pd, prob_lo, prob_hi, time, dx)
    else
       call vamd_write_d(v, rrs(1:nr), dirname, names, prob_lo=prob_lo, prob_hi=prob_hi, time=time, dx=dx)
    end if
  end subroutine fabio_ml_multifab_write_d

  ! fabio_ml_multifab_read_d(mfs, dirname)   (src/checkpoint.f90:130,134): allocates mfs(1:nlevs), builds the layout from the file's box lists (problem domain:
  ! the bounding box of level 1, refined) and the multifabs with the file's components and nodal flags and no ghost cells, then reads the data
  subroutine fabio_ml_multifab_read_d(mfs, dirname)
    type(multifab), pointer :: mfs(:)
    character(len=*), intent(in) :: dirname
    type(ml_boxarray) :: mba
    type(vdn_box), allocatable :: vb(:)
    type(box), allocatable :: bxs(:)
    type(vamd_multifab), allocatable :: v(:)
    integer :: nlev, dm, nc, nb(4), rr(4), n, i
    logical :: nodal(3)
    real(dp_t) :: time
    call vamd_info(dirname, nlev, dm, nc, nodal, nb, rr, time)
    if (nread >= size(read_mla)) error stop 'fabio_ml_multifab_read_d: more than 16 hierarchies read in one run'
    nread = nread + 1
    call ml_boxarray_build_n(mba, nlev, dm)
    do n = 1, nlev
       allocate(vb(nb(n)), bxs(nb(n)))
       call vamd_boxes(dirname, n, vb)
       do i = 1, nb(n)
          bxs(i)%dim = dm; bxs(i)%lo = vb(i)%lo; bxs(i)%hi = vb(i)%hi
       end do
       call boxarray_build_v(mba%bas(n), bxs)
       if (n == 1) then
          mba%pd(1)%dim = dm
          do i = 1, 3
             mba%pd(1)%lo(i) = minval(vb%lo(i)); mba%pd(1)%hi(i) = maxval(vb%hi(i))
          end do
       else
          mba%rr(n - 1, :) = rr(n - 1)
          mba%pd(n) = mba%pd(n - 1)
          mba%pd(n)%lo(1:dm) = mba%pd(n - 1)%lo(1:dm) * rr(n - 1); mba%pd(n)%hi(1:dm) = (mba%pd(n - 1)%hi(1:dm) + 1) * rr(n - 1) - 1
       end if
       deallocate(vb, bxs)
    end do
    call ml_layout_build(read_mla(nread), mba)
    call destroy(mba)
    allocate(mfs(nlev), v(nlev))
    do n = 1, nlev
       call multifab_build(mfs(n), read_mla(nread)%la(n), nc, 0, nodal(1:dm))
       v(n) = mfs(n)%v
    end do
    call vamd_read_d(v, dirname)
  end subroutine fabio_ml_multifab_read_d
end module fabio_module

! plane-averaged profiles of a hierarchy along one axis on the reference's container types (no reference counterpart; include/varden_amd.h: vdn_profiles):
! profiles_layout(dm, nscal, lay) and type(vdn_profile_layout) as in varden_amd, profiles_nbins(mla, axis), profiles(mla, u, s, dx, axis, out, cells) with
! out(nbins, nrow), cells(nbins); axis numbered from 1
module profiles_module
  use iso_c_binding, only: c_long_long
  use multifab_module
  use ml_layout_module
  use varden_amd, only: vdn_profile_layout, profiles_layout, vamd_profiles_nbins => profiles_nbins, vamd_profiles => profiles, vamd_multifab => multifab
  implicit none
contains
  function profiles_nbins(mla, axis) result(nbins)
    type(ml_layout), intent(in) :: mla
    integer, intent(in) :: axis
    integer :: nbins
    nbins = vamd_profiles_nbins(mla%v, mla%nlevel, axis)
  end function profiles_nbins
  subroutine profiles(mla, u, s, dx, axis, out, cells)
    type(ml_layout), intent(in   ) :: mla
    type(multifab) , intent(in   ) :: u(:), s(:)
    real(dp_t)     , intent(in   ) :: dx(:,:)
    integer        , intent(in   ) :: axis
    real(dp_t)     , intent(  out) :: out(:,:)
    integer(c_long_long), intent(out) :: cells(:)
    type(vamd_multifab) :: uv(size(u)), sv(size(s))
    integer :: n
    do n = 1, size(u)
       uv(n) = u(n)%v; sv(n) = s(n)%v
    end do
    call vamd_profiles(mla%v, uv, sv, dx, axis, out, cells)
  end subroutine profiles
end module profiles_module
