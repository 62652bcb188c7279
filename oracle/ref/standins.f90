! oracle/ref/standins.f90 -- stand-ins for the five declaration-only modules that the reference's
! array-level routines `use`.  TEST INFRASTRUCTURE ONLY.  Written from nothing: a kind, named
! constants, the integer names of the boundary types (the values of include/varden_amd.h), an error
! hook, and the handful of run-time parameters the routines read.  No text of the reference.

module bl_types
  implicit none
  integer, parameter :: dp_t = kind(1.0d0)
end module bl_types

module bl_constants_module
  use bl_types
  implicit none
  real(dp_t), parameter :: ZERO = 0.0_dp_t, ONE = 1.0_dp_t, TWO = 2.0_dp_t, THREE = 3.0_dp_t
  real(dp_t), parameter :: FOUR = 4.0_dp_t, FIVE = 5.0_dp_t, SIX = 6.0_dp_t, SEVEN = 7.0_dp_t
  real(dp_t), parameter :: EIGHT = 8.0_dp_t, NINE = 9.0_dp_t, TEN = 10.0_dp_t, ELEVEN = 11.0_dp_t
  real(dp_t), parameter :: TWELVE = 12.0_dp_t, FIFTEEN = 15.0_dp_t, SIXTEEN = 16.0_dp_t
  real(dp_t), parameter :: HALF = 0.5_dp_t, THIRD = 1.0_dp_t / 3.0_dp_t, FOURTH = 0.25_dp_t
  real(dp_t), parameter :: FIFTH = 0.2_dp_t, SIXTH = 1.0_dp_t / 6.0_dp_t, SEVENTH = 1.0_dp_t / 7.0_dp_t
  real(dp_t), parameter :: EIGHTH = 0.125_dp_t, TENTH = 0.1_dp_t, TWO3RD = 2.0_dp_t / 3.0_dp_t
end module bl_constants_module

module bc_module
  implicit none
  integer, parameter :: PERIODIC = -1, INTERIOR = 0
  integer, parameter :: INLET = 11, OUTLET = 12, SYMMETRY = 13, SLIP_WALL = 14, NO_SLIP_WALL = 15
  integer, parameter :: REFLECT_ODD = 20, REFLECT_EVEN = 21, FOEXTRAP = 22, EXT_DIR = 23, HOEXTRAP = 24
end module bc_module

module bl_error_module
  implicit none
  integer, save :: vref_nerr = 0      ! calls of bl_error since the last reset (the caller reads it; nothing stops)
contains
  subroutine bl_error(str)
    character(len=*), intent(in) :: str
    vref_nerr = vref_nerr + 1
  end subroutine bl_error
end module bl_error_module

module probin_module
  use bl_types
  implicit none
  integer,    save :: slope_order = 4, boussinesq = 0, nscal = 2, extrap_comp = 0, prob_type = 1, verbose = 0
  logical,    save :: use_minion = .false.
  real(dp_t), save :: visc_coef = 0.0_dp_t, diff_coef = 0.0_dp_t
  real(dp_t), save :: rho_bc(3,2) = 0.0_dp_t, trac_bc(3,2) = 0.0_dp_t
  real(dp_t), save :: u_bc(3,2) = 0.0_dp_t, v_bc(3,2) = 0.0_dp_t, w_bc(3,2) = 0.0_dp_t
end module probin_module
