!> GPU test of the Fortran wrappers of the two-steps-per-call distributed shallow-water entries
!! (tests/test_gpu_fortran_x2_dm.py).  Mode "same": a one-rank grid decomposed with halo_width = 2, whose wrappers pass the C
!! entries a plan without messages (serial_plan_for): invoke_shallow_step_x2_dm must equal invoke_shallow_step_x2, and
!! invoke_shallow_step_smooth_x2_dm must equal invoke_shallow_step_smooth_x2, bit for bit, in every field.  Mode "hw1": the same call on a halo_width = 1 grid must stop.
!!   ftest_x2_dm.exe NX NY same|hw1
program ftest_x2_dm
  use iso_c_binding
  use kind_params_mod
  use parallel_mod
  use grid_mod
  use field_mod
  use gocean_mod
  use dlesm_psy_mod
  implicit none
  character(len=32) :: arg, mode
  integer :: nx, ny, k, ndiff
  type(grid_type), target :: g
  type(r2d_field), target :: a(12), b(12)
  type(c_sw_params) :: prm
  real(go_wp), parameter :: alpha = 0.1_go_wp

  call get_command_argument(1, arg); read(arg, *) nx
  call get_command_argument(2, arg); read(arg, *) ny
  call get_command_argument(3, mode)
  call gocean_initialise()
  g = grid_type(GO_ARAKAWA_C, (/GO_BC_EXTERNAL, GO_BC_EXTERNAL, GO_BC_NONE/), GO_OFFSET_NE)
  if (trim(mode) == 'hw1') then
     call g%decompose(nx, ny, halo_width=1)
  else
     call g%decompose(nx, ny, halo_width=2)
  end if
  call grid_init(g, 1.0e5_go_wp, 1.0e5_go_wp)
  prm = shallow_params(g%dx, g%dy, 90.0_go_wp)

  ! plain form: a = the distributed entry, b = the single-domain entry, from the same twelve fields
  call init_sets()
  call invoke_shallow_step_x2_dm(prm, a(1), a(2), a(3), a(4), a(5), a(6), a(7), a(8), a(9), a(10), a(11), a(12))
  call invoke_shallow_step_x2(prm, b(1), b(2), b(3), b(4), b(5), b(6), b(7), b(8), b(9), b(10), b(11), b(12))
  write(*, '("G: x2 ",i0)') count_diff()
  ! filtered form
  call init_sets()
  call invoke_shallow_step_smooth_x2_dm(prm, alpha, a(1), a(2), a(3), a(4), a(5), a(6), a(7), a(8), a(9), a(10), a(11), a(12))
  call invoke_shallow_step_smooth_x2(prm, alpha, b(1), b(2), b(3), b(4), b(5), b(6), b(7), b(8), b(9), b(10), b(11), b(12))
  write(*, '("G: smooth_x2 ",i0)') count_diff()
  call gocean_finalise()

contains

  subroutine init_sets()
    integer :: pt
    do k = 1, 12
       select case (mod(k - 1, 3))
       case (0); pt = GO_U_POINTS
       case (1); pt = GO_V_POINTS
       case default; pt = GO_T_POINTS
       end select
       if (.not. allocated(a(k)%data)) then
          a(k) = r2d_field(g, pt)
          b(k) = r2d_field(g, pt)
       end if
       call invoke_hash_init(a(k), int(1000 + k, c_int64_t))
       call a(k)%read_from_device()
       if (pt == GO_T_POINTS) then
          a(k)%data = 1.0_go_wp + 0.01_go_wp * a(k)%data
       else
          a(k)%data = 0.01_go_wp * a(k)%data - 0.005_go_wp
       end if
       call a(k)%write_to_device()
       call invoke_copy(b(k), a(k))
    end do
    call device_sync()
  end subroutine init_sets

  integer function count_diff()
    count_diff = 0
    call device_sync()
    do k = 1, 12
       call a(k)%read_from_device()
       call b(k)%read_from_device()
       ndiff = count(a(k)%data /= b(k)%data)
       if (ndiff /= 0) write(*, '("G: field ",i0," differs in ",i0," cells")') k, ndiff
       count_diff = count_diff + ndiff
    end do
  end function count_diff

end program ftest_x2_dm
