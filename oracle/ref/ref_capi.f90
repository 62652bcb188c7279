! oracle/ref/ref_capi.f90 -- C entry points to the reference's own array-level routines (module
! ref_kernels: their text, cut out of the reference tree at build time and compiled unmodified;
! slope_module: the reference's slope.f90 as a whole).  TEST INFRASTRUCTURE ONLY.
! The wrappers declare the bounds of the arrays they are handed (Fortran order, the caller makes the
! copy), turn integer flags into logicals, and call.  lo, hi are the valid cell box; ng_* ghost widths.

module vref_capi
  use iso_c_binding
  use bl_types
  use bl_error_module, only: vref_nerr
  use slope_module
  use ref_kernels
  implicit none
contains

  subroutine vref_set_probin(slope_order_, use_minion_, boussinesq_, visc_coef_, diff_coef_, nscal_, extrap_comp_, &
                             prob_type_, u_bc_, v_bc_, w_bc_, rho_bc_, trac_bc_) bind(C, name="vref_set_probin")
    use probin_module
    integer(c_int), value :: slope_order_, use_minion_, boussinesq_, nscal_, extrap_comp_, prob_type_
    real(c_double), value :: visc_coef_, diff_coef_
    real(c_double), intent(in) :: u_bc_(3,2), v_bc_(3,2), w_bc_(3,2), rho_bc_(3,2), trac_bc_(3,2)
    slope_order = slope_order_; use_minion = use_minion_ /= 0; boussinesq = boussinesq_
    visc_coef = visc_coef_; diff_coef = diff_coef_; nscal = nscal_; extrap_comp = extrap_comp_; prob_type = prob_type_
    u_bc = u_bc_; v_bc = v_bc_; w_bc = w_bc_; rho_bc = rho_bc_; trac_bc = trac_bc_
  end subroutine vref_set_probin

  ! calls of bl_error since the last call of this function
  function vref_errors() bind(C, name="vref_errors") result(n)
    integer(c_int) :: n
    n = vref_nerr
    vref_nerr = 0
  end function vref_errors

  ! ---- slopes: dir = 1, 2, 3.  In 3-D the x and y slopes are taken plane by plane over k = lo(3)-1 .. hi(3)+1, which is how
  !      the reference's 3-D callers obtain them; bc is adv_bc(dm,2,nvar) ----
  subroutine vref_slope_3d(dir, s, sl, lo, hi, ng_s, ng_o, nvar, bc) bind(C, name="vref_slope_3d")
    integer(c_int), value :: dir, ng_s, ng_o, nvar
    integer(c_int), intent(in) :: lo(3), hi(3), bc(3,2,nvar)
    real(c_double), intent(in)    ::  s(lo(1)-ng_s:hi(1)+ng_s, lo(2)-ng_s:hi(2)+ng_s, lo(3)-ng_s:hi(3)+ng_s, nvar)
    real(c_double), intent(inout) :: sl(lo(1)-ng_o:hi(1)+ng_o, lo(2)-ng_o:hi(2)+ng_o, lo(3)-ng_o:hi(3)+ng_o, nvar)
    integer :: k
    if (dir == 3) then
       call slopez_3d(s, sl, lo, hi, ng_s, ng_o, nvar, bc)
    else
       do k = lo(3)-1, hi(3)+1
          if (dir == 1) call slopex_2d(s(:,:,k,:), sl(:,:,k,:), lo, hi, ng_s, ng_o, nvar, bc)
          if (dir == 2) call slopey_2d(s(:,:,k,:), sl(:,:,k,:), lo, hi, ng_s, ng_o, nvar, bc)
       end do
    end if
  end subroutine vref_slope_3d

  subroutine vref_slope_2d(dir, s, sl, lo, hi, ng_s, ng_o, nvar, bc) bind(C, name="vref_slope_2d")
    integer(c_int), value :: dir, ng_s, ng_o, nvar
    integer(c_int), intent(in) :: lo(2), hi(2), bc(2,2,nvar)
    real(c_double), intent(in)    ::  s(lo(1)-ng_s:hi(1)+ng_s, lo(2)-ng_s:hi(2)+ng_s, nvar)
    real(c_double), intent(inout) :: sl(lo(1)-ng_o:hi(1)+ng_o, lo(2)-ng_o:hi(2)+ng_o, nvar)
    if (dir == 1) call slopex_2d(s, sl, lo, hi, ng_s, ng_o, nvar, bc)
    if (dir == 2) call slopey_2d(s, sl, lo, hi, ng_s, ng_o, nvar, bc)
  end subroutine vref_slope_2d

  ! ---- velpred: adv_bc is the whole table adv_bc(dm,2,nbc) ----
  subroutine vref_velpred_3d(u, umac, vmac, wmac, force, lo, hi, dx, dt, phys_bc, adv_bc, nbc, ng_u, ng_m, ng_f) &
       bind(C, name="vref_velpred_3d")
    integer(c_int), value :: nbc, ng_u, ng_m, ng_f
    real(c_double), value :: dt
    integer(c_int), intent(in) :: lo(3), hi(3), phys_bc(3,2), adv_bc(3,2,nbc)
    real(c_double), intent(in) :: dx(3)
    real(c_double), intent(in)    ::     u(lo(1)-ng_u:hi(1)+ng_u, lo(2)-ng_u:hi(2)+ng_u, lo(3)-ng_u:hi(3)+ng_u, 3)
    real(c_double), intent(inout) ::  umac(lo(1)-ng_m:hi(1)+ng_m+1, lo(2)-ng_m:hi(2)+ng_m, lo(3)-ng_m:hi(3)+ng_m)
    real(c_double), intent(inout) ::  vmac(lo(1)-ng_m:hi(1)+ng_m, lo(2)-ng_m:hi(2)+ng_m+1, lo(3)-ng_m:hi(3)+ng_m)
    real(c_double), intent(inout) ::  wmac(lo(1)-ng_m:hi(1)+ng_m, lo(2)-ng_m:hi(2)+ng_m, lo(3)-ng_m:hi(3)+ng_m+1)
    real(c_double), intent(inout) :: force(lo(1)-ng_f:hi(1)+ng_f, lo(2)-ng_f:hi(2)+ng_f, lo(3)-ng_f:hi(3)+ng_f, 3)
    call velpred_3d(u, umac, vmac, wmac, force, lo, hi, dx, dt, phys_bc, adv_bc, ng_u, ng_m, ng_f)
  end subroutine vref_velpred_3d

  subroutine vref_velpred_2d(u, umac, vmac, force, lo, hi, dx, dt, phys_bc, adv_bc, nbc, ng_u, ng_m, ng_f) &
       bind(C, name="vref_velpred_2d")
    integer(c_int), value :: nbc, ng_u, ng_m, ng_f
    real(c_double), value :: dt
    integer(c_int), intent(in) :: lo(2), hi(2), phys_bc(2,2), adv_bc(2,2,nbc)
    real(c_double), intent(in) :: dx(2)
    real(c_double), intent(in)    ::     u(lo(1)-ng_u:hi(1)+ng_u, lo(2)-ng_u:hi(2)+ng_u, 2)
    real(c_double), intent(inout) ::  umac(lo(1)-ng_m:hi(1)+ng_m+1, lo(2)-ng_m:hi(2)+ng_m)
    real(c_double), intent(inout) ::  vmac(lo(1)-ng_m:hi(1)+ng_m, lo(2)-ng_m:hi(2)+ng_m+1)
    real(c_double), intent(inout) :: force(lo(1)-ng_f:hi(1)+ng_f, lo(2)-ng_f:hi(2)+ng_f, 2)
    call velpred_2d(u, umac, vmac, force, lo, hi, dx, dt, phys_bc, adv_bc, ng_u, ng_m, ng_f)
  end subroutine vref_velpred_2d

  ! ---- mkflux: adv_bc holds the ncomp components of s only, adv_bc(dm,2,ncomp), as the reference's driver slices it ----
  subroutine vref_mkflux_3d(s, sedgex, sedgey, sedgez, fluxx, fluxy, fluxz, umac, vmac, wmac, force, mac_rhs, lo, hi, dx, dt, &
                            is_vel, phys_bc, adv_bc, ncomp, ng_s, ng_e, ng_f, ng_u, ng_o, ng_m, is_cons) bind(C, name="vref_mkflux_3d")
    integer(c_int), value :: is_vel, ncomp, ng_s, ng_e, ng_f, ng_u, ng_o, ng_m
    real(c_double), value :: dt
    integer(c_int), intent(in) :: lo(3), hi(3), phys_bc(3,2), adv_bc(3,2,ncomp), is_cons(ncomp)
    real(c_double), intent(in) :: dx(3)
    real(c_double), intent(in)    ::       s(lo(1)-ng_s:hi(1)+ng_s, lo(2)-ng_s:hi(2)+ng_s, lo(3)-ng_s:hi(3)+ng_s, ncomp)
    real(c_double), intent(inout) ::  sedgex(lo(1)-ng_e:hi(1)+ng_e+1, lo(2)-ng_e:hi(2)+ng_e, lo(3)-ng_e:hi(3)+ng_e, ncomp)
    real(c_double), intent(inout) ::  sedgey(lo(1)-ng_e:hi(1)+ng_e, lo(2)-ng_e:hi(2)+ng_e+1, lo(3)-ng_e:hi(3)+ng_e, ncomp)
    real(c_double), intent(inout) ::  sedgez(lo(1)-ng_e:hi(1)+ng_e, lo(2)-ng_e:hi(2)+ng_e, lo(3)-ng_e:hi(3)+ng_e+1, ncomp)
    real(c_double), intent(inout) ::   fluxx(lo(1)-ng_f:hi(1)+ng_f+1, lo(2)-ng_f:hi(2)+ng_f, lo(3)-ng_f:hi(3)+ng_f, ncomp)
    real(c_double), intent(inout) ::   fluxy(lo(1)-ng_f:hi(1)+ng_f, lo(2)-ng_f:hi(2)+ng_f+1, lo(3)-ng_f:hi(3)+ng_f, ncomp)
    real(c_double), intent(inout) ::   fluxz(lo(1)-ng_f:hi(1)+ng_f, lo(2)-ng_f:hi(2)+ng_f, lo(3)-ng_f:hi(3)+ng_f+1, ncomp)
    real(c_double), intent(in)    ::    umac(lo(1)-ng_u:hi(1)+ng_u+1, lo(2)-ng_u:hi(2)+ng_u, lo(3)-ng_u:hi(3)+ng_u)
    real(c_double), intent(in)    ::    vmac(lo(1)-ng_u:hi(1)+ng_u, lo(2)-ng_u:hi(2)+ng_u+1, lo(3)-ng_u:hi(3)+ng_u)
    real(c_double), intent(in)    ::    wmac(lo(1)-ng_u:hi(1)+ng_u, lo(2)-ng_u:hi(2)+ng_u, lo(3)-ng_u:hi(3)+ng_u+1)
    real(c_double), intent(in)    ::   force(lo(1)-ng_o:hi(1)+ng_o, lo(2)-ng_o:hi(2)+ng_o, lo(3)-ng_o:hi(3)+ng_o, ncomp)
    real(c_double), intent(in)    :: mac_rhs(lo(1)-ng_m:hi(1)+ng_m, lo(2)-ng_m:hi(2)+ng_m, lo(3)-ng_m:hi(3)+ng_m)
    logical :: lcons(ncomp)
    lcons = is_cons /= 0
    call mkflux_3d(s, sedgex, sedgey, sedgez, fluxx, fluxy, fluxz, umac, vmac, wmac, force, mac_rhs, lo, hi, dx, dt, &
                   is_vel /= 0, phys_bc, adv_bc, ng_s, ng_e, ng_f, ng_u, ng_o, ng_m, lcons)
  end subroutine vref_mkflux_3d

  subroutine vref_mkflux_2d(s, sedgex, sedgey, fluxx, fluxy, umac, vmac, force, mac_rhs, lo, hi, dx, dt, &
                            is_vel, phys_bc, adv_bc, ncomp, ng_s, ng_e, ng_f, ng_u, ng_o, ng_m, is_cons) bind(C, name="vref_mkflux_2d")
    integer(c_int), value :: is_vel, ncomp, ng_s, ng_e, ng_f, ng_u, ng_o, ng_m
    real(c_double), value :: dt
    integer(c_int), intent(in) :: lo(2), hi(2), phys_bc(2,2), adv_bc(2,2,ncomp), is_cons(ncomp)
    real(c_double), intent(in) :: dx(2)
    real(c_double), intent(in)    ::       s(lo(1)-ng_s:hi(1)+ng_s, lo(2)-ng_s:hi(2)+ng_s, ncomp)
    real(c_double), intent(inout) ::  sedgex(lo(1)-ng_e:hi(1)+ng_e+1, lo(2)-ng_e:hi(2)+ng_e, ncomp)
    real(c_double), intent(inout) ::  sedgey(lo(1)-ng_e:hi(1)+ng_e, lo(2)-ng_e:hi(2)+ng_e+1, ncomp)
    real(c_double), intent(inout) ::   fluxx(lo(1)-ng_f:hi(1)+ng_f+1, lo(2)-ng_f:hi(2)+ng_f, ncomp)
    real(c_double), intent(inout) ::   fluxy(lo(1)-ng_f:hi(1)+ng_f, lo(2)-ng_f:hi(2)+ng_f+1, ncomp)
    real(c_double), intent(in)    ::    umac(lo(1)-ng_u:hi(1)+ng_u+1, lo(2)-ng_u:hi(2)+ng_u)
    real(c_double), intent(in)    ::    vmac(lo(1)-ng_u:hi(1)+ng_u, lo(2)-ng_u:hi(2)+ng_u+1)
    real(c_double), intent(in)    ::   force(lo(1)-ng_o:hi(1)+ng_o, lo(2)-ng_o:hi(2)+ng_o, ncomp)
    real(c_double), intent(in)    :: mac_rhs(lo(1)-ng_m:hi(1)+ng_m, lo(2)-ng_m:hi(2)+ng_m)
    logical :: lcons(ncomp)
    lcons = is_cons /= 0
    call mkflux_2d(s, sedgex, sedgey, fluxx, fluxy, umac, vmac, force, mac_rhs, lo, hi, dx, dt, &
                   is_vel /= 0, phys_bc, adv_bc, ng_s, ng_e, ng_f, ng_u, ng_o, ng_m, lcons)
  end subroutine vref_mkflux_2d

  ! ---- update ----
  subroutine vref_update_3d(sold, umac, vmac, wmac, sedgex, sedgey, sedgez, fluxx, fluxy, fluxz, force, snew, lo, hi, &
                            ncomp, ng_s, ng_u, ng_e, ng_f, ng_o, dx, dt, is_vel, is_cons) bind(C, name="vref_update_3d")
    integer(c_int), value :: is_vel, ncomp, ng_s, ng_u, ng_e, ng_f, ng_o
    real(c_double), value :: dt
    integer(c_int), intent(in) :: lo(3), hi(3), is_cons(ncomp)
    real(c_double), intent(in) :: dx(3)
    real(c_double), intent(in)    ::    sold(lo(1)-ng_s:hi(1)+ng_s, lo(2)-ng_s:hi(2)+ng_s, lo(3)-ng_s:hi(3)+ng_s, ncomp)
    real(c_double), intent(inout) ::    snew(lo(1)-ng_s:hi(1)+ng_s, lo(2)-ng_s:hi(2)+ng_s, lo(3)-ng_s:hi(3)+ng_s, ncomp)
    real(c_double), intent(in)    ::    umac(lo(1)-ng_u:hi(1)+ng_u+1, lo(2)-ng_u:hi(2)+ng_u, lo(3)-ng_u:hi(3)+ng_u)
    real(c_double), intent(in)    ::    vmac(lo(1)-ng_u:hi(1)+ng_u, lo(2)-ng_u:hi(2)+ng_u+1, lo(3)-ng_u:hi(3)+ng_u)
    real(c_double), intent(in)    ::    wmac(lo(1)-ng_u:hi(1)+ng_u, lo(2)-ng_u:hi(2)+ng_u, lo(3)-ng_u:hi(3)+ng_u+1)
    real(c_double), intent(in)    ::  sedgex(lo(1)-ng_e:hi(1)+ng_e+1, lo(2)-ng_e:hi(2)+ng_e, lo(3)-ng_e:hi(3)+ng_e, ncomp)
    real(c_double), intent(in)    ::  sedgey(lo(1)-ng_e:hi(1)+ng_e, lo(2)-ng_e:hi(2)+ng_e+1, lo(3)-ng_e:hi(3)+ng_e, ncomp)
    real(c_double), intent(in)    ::  sedgez(lo(1)-ng_e:hi(1)+ng_e, lo(2)-ng_e:hi(2)+ng_e, lo(3)-ng_e:hi(3)+ng_e+1, ncomp)
    real(c_double), intent(in)    ::   fluxx(lo(1)-ng_f:hi(1)+ng_f+1, lo(2)-ng_f:hi(2)+ng_f, lo(3)-ng_f:hi(3)+ng_f, ncomp)
    real(c_double), intent(in)    ::   fluxy(lo(1)-ng_f:hi(1)+ng_f, lo(2)-ng_f:hi(2)+ng_f+1, lo(3)-ng_f:hi(3)+ng_f, ncomp)
    real(c_double), intent(in)    ::   fluxz(lo(1)-ng_f:hi(1)+ng_f, lo(2)-ng_f:hi(2)+ng_f, lo(3)-ng_f:hi(3)+ng_f+1, ncomp)
    real(c_double), intent(in)    ::   force(lo(1)-ng_o:hi(1)+ng_o, lo(2)-ng_o:hi(2)+ng_o, lo(3)-ng_o:hi(3)+ng_o, ncomp)
    logical :: lcons(ncomp)
    lcons = is_cons /= 0
    call update_3d(sold, umac, vmac, wmac, sedgex, sedgey, sedgez, fluxx, fluxy, fluxz, force, snew, lo, hi, &
                   ng_s, ng_u, ng_e, ng_f, ng_o, dx, dt, is_vel /= 0, lcons)
  end subroutine vref_update_3d

  subroutine vref_update_2d(sold, umac, vmac, sedgex, sedgey, fluxx, fluxy, force, snew, lo, hi, &
                            ncomp, ng_s, ng_u, ng_e, ng_f, ng_o, dx, dt, is_vel, is_cons) bind(C, name="vref_update_2d")
    integer(c_int), value :: is_vel, ncomp, ng_s, ng_u, ng_e, ng_f, ng_o
    real(c_double), value :: dt
    integer(c_int), intent(in) :: lo(2), hi(2), is_cons(ncomp)
    real(c_double), intent(in) :: dx(2)
    real(c_double), intent(in)    ::    sold(lo(1)-ng_s:hi(1)+ng_s, lo(2)-ng_s:hi(2)+ng_s, ncomp)
    real(c_double), intent(inout) ::    snew(lo(1)-ng_s:hi(1)+ng_s, lo(2)-ng_s:hi(2)+ng_s, ncomp)
    real(c_double), intent(in)    ::    umac(lo(1)-ng_u:hi(1)+ng_u+1, lo(2)-ng_u:hi(2)+ng_u)
    real(c_double), intent(in)    ::    vmac(lo(1)-ng_u:hi(1)+ng_u, lo(2)-ng_u:hi(2)+ng_u+1)
    real(c_double), intent(in)    ::  sedgex(lo(1)-ng_e:hi(1)+ng_e+1, lo(2)-ng_e:hi(2)+ng_e, ncomp)
    real(c_double), intent(in)    ::  sedgey(lo(1)-ng_e:hi(1)+ng_e, lo(2)-ng_e:hi(2)+ng_e+1, ncomp)
    real(c_double), intent(in)    ::   fluxx(lo(1)-ng_f:hi(1)+ng_f+1, lo(2)-ng_f:hi(2)+ng_f, ncomp)
    real(c_double), intent(in)    ::   fluxy(lo(1)-ng_f:hi(1)+ng_f, lo(2)-ng_f:hi(2)+ng_f+1, ncomp)
    real(c_double), intent(in)    ::   force(lo(1)-ng_o:hi(1)+ng_o, lo(2)-ng_o:hi(2)+ng_o, ncomp)
    logical :: lcons(ncomp)
    lcons = is_cons /= 0
    call update_2d(sold, umac, vmac, sedgex, sedgey, fluxx, fluxy, force, snew, lo, hi, &
                   ng_s, ng_u, ng_e, ng_f, ng_o, dx, dt, is_vel /= 0, lcons)
  end subroutine vref_update_2d

  ! ---- forces: ns = components of s; the scalar forces carry probin's nscal components ----
  subroutine vref_mkvelforce_3d(vel_force, ext, gp, s, lapu, ns, ng_f, ng_e, ng_g, ng_s, ng_l, visc_fac, lo, hi) &
       bind(C, name="vref_mkvelforce_3d")
    integer(c_int), value :: ns, ng_f, ng_e, ng_g, ng_s, ng_l
    real(c_double), value :: visc_fac
    integer(c_int), intent(in) :: lo(3), hi(3)
    real(c_double), intent(inout) :: vel_force(lo(1)-ng_f:hi(1)+ng_f, lo(2)-ng_f:hi(2)+ng_f, lo(3)-ng_f:hi(3)+ng_f, 3)
    real(c_double), intent(in)    ::       ext(lo(1)-ng_e:hi(1)+ng_e, lo(2)-ng_e:hi(2)+ng_e, lo(3)-ng_e:hi(3)+ng_e, 3)
    real(c_double), intent(in)    ::        gp(lo(1)-ng_g:hi(1)+ng_g, lo(2)-ng_g:hi(2)+ng_g, lo(3)-ng_g:hi(3)+ng_g, 3)
    real(c_double), intent(in)    ::         s(lo(1)-ng_s:hi(1)+ng_s, lo(2)-ng_s:hi(2)+ng_s, lo(3)-ng_s:hi(3)+ng_s, ns)
    real(c_double), intent(in)    ::      lapu(lo(1)-ng_l:hi(1)+ng_l, lo(2)-ng_l:hi(2)+ng_l, lo(3)-ng_l:hi(3)+ng_l, 3)
    call mkvelforce_3d(vel_force, ext, gp, s, lapu, ng_f, ng_e, ng_g, ng_s, ng_l, visc_fac, lo, hi)
  end subroutine vref_mkvelforce_3d

  subroutine vref_mkvelforce_2d(vel_force, ext, gp, s, lapu, ns, ng_f, ng_e, ng_g, ng_s, ng_l, visc_fac, lo, hi) &
       bind(C, name="vref_mkvelforce_2d")
    integer(c_int), value :: ns, ng_f, ng_e, ng_g, ng_s, ng_l
    real(c_double), value :: visc_fac
    integer(c_int), intent(in) :: lo(2), hi(2)
    real(c_double), intent(inout) :: vel_force(lo(1)-ng_f:hi(1)+ng_f, lo(2)-ng_f:hi(2)+ng_f, 2)
    real(c_double), intent(in)    ::       ext(lo(1)-ng_e:hi(1)+ng_e, lo(2)-ng_e:hi(2)+ng_e, 2)
    real(c_double), intent(in)    ::        gp(lo(1)-ng_g:hi(1)+ng_g, lo(2)-ng_g:hi(2)+ng_g, 2)
    real(c_double), intent(in)    ::         s(lo(1)-ng_s:hi(1)+ng_s, lo(2)-ng_s:hi(2)+ng_s, ns)
    real(c_double), intent(in)    ::      lapu(lo(1)-ng_l:hi(1)+ng_l, lo(2)-ng_l:hi(2)+ng_l, 2)
    call mkvelforce_2d(vel_force, ext, gp, s, lapu, ng_f, ng_e, ng_g, ng_s, ng_l, visc_fac, lo, hi)
  end subroutine vref_mkvelforce_2d

  subroutine vref_mkscalforce_3d(scal_force, ext, laps, ns, ng_f, ng_e, ng_l, diff_fac, lo, hi) bind(C, name="vref_mkscalforce_3d")
    integer(c_int), value :: ns, ng_f, ng_e, ng_l
    real(c_double), value :: diff_fac
    integer(c_int), intent(in) :: lo(3), hi(3)
    real(c_double), intent(inout) :: scal_force(lo(1)-ng_f:hi(1)+ng_f, lo(2)-ng_f:hi(2)+ng_f, lo(3)-ng_f:hi(3)+ng_f, ns)
    real(c_double), intent(in)    ::        ext(lo(1)-ng_e:hi(1)+ng_e, lo(2)-ng_e:hi(2)+ng_e, lo(3)-ng_e:hi(3)+ng_e, ns)
    real(c_double), intent(in)    ::       laps(lo(1)-ng_l:hi(1)+ng_l, lo(2)-ng_l:hi(2)+ng_l, lo(3)-ng_l:hi(3)+ng_l, ns)
    call mkscalforce_3d(scal_force, ext, laps, ng_f, ng_e, ng_l, diff_fac, lo, hi)
  end subroutine vref_mkscalforce_3d

  subroutine vref_mkscalforce_2d(scal_force, ext, laps, ns, ng_f, ng_e, ng_l, diff_fac, lo, hi) bind(C, name="vref_mkscalforce_2d")
    integer(c_int), value :: ns, ng_f, ng_e, ng_l
    real(c_double), value :: diff_fac
    integer(c_int), intent(in) :: lo(2), hi(2)
    real(c_double), intent(inout) :: scal_force(lo(1)-ng_f:hi(1)+ng_f, lo(2)-ng_f:hi(2)+ng_f, ns)
    real(c_double), intent(in)    ::        ext(lo(1)-ng_e:hi(1)+ng_e, lo(2)-ng_e:hi(2)+ng_e, ns)
    real(c_double), intent(in)    ::       laps(lo(1)-ng_l:hi(1)+ng_l, lo(2)-ng_l:hi(2)+ng_l, ns)
    call mkscalforce_2d(scal_force, ext, laps, ng_f, ng_e, ng_l, diff_fac, lo, hi)
  end subroutine vref_mkscalforce_2d

  ! ---- estdt: the per-box kernel; dt goes in as the caller's starting value and comes back lowered; s is the density alone ----
  subroutine vref_estdt_3d(vel, ng_u, s, ng_s, gp, ng_g, ext, ng_f, lo, hi, dx, dt) bind(C, name="vref_estdt_3d")
    integer(c_int), value :: ng_u, ng_s, ng_g, ng_f
    integer(c_int), intent(in) :: lo(3), hi(3)
    real(c_double), intent(in) :: dx(3)
    real(c_double), intent(inout) :: dt
    real(c_double), intent(in) :: vel(lo(1)-ng_u:hi(1)+ng_u, lo(2)-ng_u:hi(2)+ng_u, lo(3)-ng_u:hi(3)+ng_u, 3)
    real(c_double), intent(in) ::   s(lo(1)-ng_s:hi(1)+ng_s, lo(2)-ng_s:hi(2)+ng_s, lo(3)-ng_s:hi(3)+ng_s)
    real(c_double), intent(in) ::  gp(lo(1)-ng_g:hi(1)+ng_g, lo(2)-ng_g:hi(2)+ng_g, lo(3)-ng_g:hi(3)+ng_g, 3)
    real(c_double), intent(in) :: ext(lo(1)-ng_f:hi(1)+ng_f, lo(2)-ng_f:hi(2)+ng_f, lo(3)-ng_f:hi(3)+ng_f, 3)
    call estdt_3d(vel, ng_u, s, ng_s, gp, ng_g, ext, ng_f, lo, hi, dx, dt)
  end subroutine vref_estdt_3d

  subroutine vref_estdt_2d(vel, ng_u, s, ng_s, gp, ng_g, ext, ng_f, lo, hi, dx, dt) bind(C, name="vref_estdt_2d")
    integer(c_int), value :: ng_u, ng_s, ng_g, ng_f
    integer(c_int), intent(in) :: lo(2), hi(2)
    real(c_double), intent(in) :: dx(2)
    real(c_double), intent(inout) :: dt
    real(c_double), intent(in) :: vel(lo(1)-ng_u:hi(1)+ng_u, lo(2)-ng_u:hi(2)+ng_u, 2)
    real(c_double), intent(in) ::   s(lo(1)-ng_s:hi(1)+ng_s, lo(2)-ng_s:hi(2)+ng_s)
    real(c_double), intent(in) ::  gp(lo(1)-ng_g:hi(1)+ng_g, lo(2)-ng_g:hi(2)+ng_g, 2)
    real(c_double), intent(in) :: ext(lo(1)-ng_f:hi(1)+ng_f, lo(2)-ng_f:hi(2)+ng_f, 2)
    call estdt_2d(vel, ng_u, s, ng_s, gp, ng_g, ext, ng_f, lo, hi, dx, dt)
  end subroutine vref_estdt_2d

  ! ---- physbc: one component; bc = adv_bc(dm,2) of that component, icomp its 1-based number ----
  subroutine vref_physbc_3d(s, lo, hi, ng, bc, icomp) bind(C, name="vref_physbc_3d")
    integer(c_int), value :: ng, icomp
    integer(c_int), intent(in) :: lo(3), hi(3), bc(3,2)
    real(c_double), intent(inout) :: s(lo(1)-ng:hi(1)+ng, lo(2)-ng:hi(2)+ng, lo(3)-ng:hi(3)+ng)
    call physbc_3d(s, lo, hi, ng, bc, icomp)
  end subroutine vref_physbc_3d

  subroutine vref_physbc_2d(s, lo, hi, ng, bc, icomp) bind(C, name="vref_physbc_2d")
    integer(c_int), value :: ng, icomp
    integer(c_int), intent(in) :: lo(2), hi(2), bc(2,2)
    real(c_double), intent(inout) :: s(lo(1)-ng:hi(1)+ng, lo(2)-ng:hi(2)+ng)
    call physbc_2d(s, lo, hi, ng, bc, icomp)
  end subroutine vref_physbc_2d

  ! ---- make_at_halftime: one component of each array ----
  subroutine vref_make_at_halftime_3d(rhohalf, rhoold, rhonew, lo, hi, ng_half, ng_old) bind(C, name="vref_make_at_halftime_3d")
    integer(c_int), value :: ng_half, ng_old
    integer(c_int), intent(in) :: lo(3), hi(3)
    real(c_double), intent(inout) :: rhohalf(lo(1)-ng_half:hi(1)+ng_half, lo(2)-ng_half:hi(2)+ng_half, lo(3)-ng_half:hi(3)+ng_half)
    real(c_double), intent(in)    ::  rhoold(lo(1)-ng_old:hi(1)+ng_old, lo(2)-ng_old:hi(2)+ng_old, lo(3)-ng_old:hi(3)+ng_old)
    real(c_double), intent(in)    ::  rhonew(lo(1)-ng_old:hi(1)+ng_old, lo(2)-ng_old:hi(2)+ng_old, lo(3)-ng_old:hi(3)+ng_old)
    call make_at_halftime_3d(rhohalf, rhoold, rhonew, lo, hi, ng_half, ng_old)
  end subroutine vref_make_at_halftime_3d

  subroutine vref_make_at_halftime_2d(rhohalf, rhoold, rhonew, lo, hi, ng_half, ng_old) bind(C, name="vref_make_at_halftime_2d")
    integer(c_int), value :: ng_half, ng_old
    integer(c_int), intent(in) :: lo(2), hi(2)
    real(c_double), intent(inout) :: rhohalf(lo(1)-ng_half:hi(1)+ng_half, lo(2)-ng_half:hi(2)+ng_half)
    real(c_double), intent(in)    ::  rhoold(lo(1)-ng_old:hi(1)+ng_old, lo(2)-ng_old:hi(2)+ng_old)
    real(c_double), intent(in)    ::  rhonew(lo(1)-ng_old:hi(1)+ng_old, lo(2)-ng_old:hi(2)+ng_old)
    call make_at_halftime_2d(rhohalf, rhoold, rhonew, lo, hi, ng_half, ng_old)
  end subroutine vref_make_at_halftime_2d

  ! ---- plot quantities: vort / magvel have no ghost cells; bc = phys_bc(dm,2) ----
  subroutine vref_makevort_3d(vort, u, lo, hi, ng, dx, bc) bind(C, name="vref_makevort_3d")
    integer(c_int), value :: ng
    integer(c_int), intent(in) :: lo(3), hi(3), bc(3,2)
    real(c_double), intent(in) :: dx(3)
    real(c_double), intent(inout) :: vort(lo(1):hi(1), lo(2):hi(2), lo(3):hi(3))
    real(c_double), intent(in)    ::    u(lo(1)-ng:hi(1)+ng, lo(2)-ng:hi(2)+ng, lo(3)-ng:hi(3)+ng, 3)
    call makevort_3d(vort, u, lo, hi, ng, dx, bc)
  end subroutine vref_makevort_3d

  subroutine vref_makevort_2d(vort, u, lo, hi, ng, dx, bc) bind(C, name="vref_makevort_2d")
    integer(c_int), value :: ng
    integer(c_int), intent(in) :: lo(2), hi(2), bc(2,2)
    real(c_double), intent(in) :: dx(2)
    real(c_double), intent(inout) :: vort(lo(1):hi(1), lo(2):hi(2))
    real(c_double), intent(in)    ::    u(lo(1)-ng:hi(1)+ng, lo(2)-ng:hi(2)+ng, 2)
    call makevort_2d(vort, u, lo, hi, ng, dx, bc)
  end subroutine vref_makevort_2d

  subroutine vref_makemagvel_3d(magvel, u, lo, hi, ng) bind(C, name="vref_makemagvel_3d")
    integer(c_int), value :: ng
    integer(c_int), intent(in) :: lo(3), hi(3)
    real(c_double), intent(inout) :: magvel(lo(1):hi(1), lo(2):hi(2), lo(3):hi(3))
    real(c_double), intent(in)    ::      u(lo(1)-ng:hi(1)+ng, lo(2)-ng:hi(2)+ng, lo(3)-ng:hi(3)+ng, 3)
    call makemagvel_3d(magvel, u, lo, hi, ng)
  end subroutine vref_makemagvel_3d

  subroutine vref_makemagvel_2d(magvel, u, lo, hi, ng) bind(C, name="vref_makemagvel_2d")
    integer(c_int), value :: ng
    integer(c_int), intent(in) :: lo(2), hi(2)
    real(c_double), intent(inout) :: magvel(lo(1):hi(1), lo(2):hi(2))
    real(c_double), intent(in)    ::      u(lo(1)-ng:hi(1)+ng, lo(2)-ng:hi(2)+ng, 2)
    call makemagvel_2d(magvel, u, lo, hi, ng)
  end subroutine vref_makemagvel_2d

  ! ---- tag_boxes: tags come back as bytes (1 = tagged) ----
  subroutine vref_tag_boxes_3d(tags, mf, lo, hi, ng, dx, lev) bind(C, name="vref_tag_boxes_3d")
    integer(c_int), value :: ng, lev
    real(c_double), value :: dx
    integer(c_int), intent(in) :: lo(3), hi(3)
    integer(c_signed_char), intent(inout) :: tags(lo(1):hi(1), lo(2):hi(2), lo(3):hi(3))
    real(c_double), intent(in) :: mf(lo(1)-ng:hi(1)+ng, lo(2)-ng:hi(2)+ng, lo(3)-ng:hi(3)+ng)
    logical :: t(lo(1):hi(1), lo(2):hi(2), lo(3):hi(3))
    call tag_boxes_3d(t, mf, lo, hi, ng, dx, lev)
    tags = merge(1_c_signed_char, 0_c_signed_char, t)
  end subroutine vref_tag_boxes_3d

  subroutine vref_tag_boxes_2d(tags, mf, lo, hi, ng, dx, lev) bind(C, name="vref_tag_boxes_2d")
    integer(c_int), value :: ng, lev
    real(c_double), value :: dx
    integer(c_int), intent(in) :: lo(2), hi(2)
    integer(c_signed_char), intent(inout) :: tags(lo(1):hi(1), lo(2):hi(2))
    real(c_double), intent(in) :: mf(lo(1)-ng:hi(1)+ng, lo(2)-ng:hi(2)+ng)
    logical :: t(lo(1):hi(1), lo(2):hi(2))
    call tag_boxes_2d(t, mf, lo, hi, ng, dx, lev)
    tags = merge(1_c_signed_char, 0_c_signed_char, t)
  end subroutine vref_tag_boxes_2d

end module vref_capi
