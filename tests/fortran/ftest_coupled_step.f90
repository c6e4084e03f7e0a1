!> GPU test of the Fortran wrappers of the coupled step on a decomposed grid, invoke_nemolite_coupled_step_dm and
!! exchange_mask_halos (tests/test_gpu_fortran_coupled_step.py).
!! Mode "dm": a one-rank grid decomposed with halo_width = 2 and a -1/0/1 user tmask, momentum_coriolis, the thirteen flow
!! fields and two tracers from invoke_hash_init; exchange_mask_halos (a plan without messages: the mask must not change), then
!! one closed-basin invoke_nemolite_coupled_step_dm with DLESM_TRACER_HANCOCK into sentinel-filled outputs; prints the array
!! extents and, per output, the bits of field_checksum and of field_stats, which the test compares with what the Python
!! wrappers invoke_nemolite_step + invoke_tracer_step_hancock leave on the same inputs.  Mode "hw1": the same call with
!! DLESM_TRACER_MUSCL on a halo_width = 1 grid must stop.
!!   ftest_coupled_step.exe NX NY dm|hw1
program ftest_coupled_step
  use iso_c_binding
  use kind_params_mod
  use parallel_mod
  use grid_mod
  use field_mod
  use gocean_mod
  use dlesm_hip_mod, only: DLESM_TRACER_MUSCL, DLESM_TRACER_HANCOCK
  use dlesm_psy_mod
  implicit none
  integer, parameter :: NF = 13
  ! 1 ssha 2 ssha_u 3 ssha_v 4 ua 5 va 6 un 7 vn 8 ht 9 hu 10 hv 11 sshn_t 12 sshn_u 13 sshn_v
  integer, parameter :: pts(NF) = (/GO_T_POINTS, GO_U_POINTS, GO_V_POINTS, GO_U_POINTS, GO_V_POINTS, GO_U_POINTS, &
                                    GO_V_POINTS, GO_T_POINTS, GO_U_POINTS, GO_V_POINTS, GO_T_POINTS, GO_U_POINTS, GO_V_POINTS/)
  character(len=8), parameter :: names(7) = (/'ssha    ', 'ssha_u  ', 'ssha_v  ', 'ua      ', 'va      ', 'c1      ', 'c2      '/)
  character(len=256) :: arg, mode
  integer :: nx, ny, i, j, k
  integer, allocatable :: tmask(:,:), before(:,:)
  type(grid_type), target :: g
  type(r2d_field), target :: f(NF), c_in(2), c_out(2)
  type(c_momentum_params) :: prm
  real(go_wp), parameter :: pi = 3.14159265358979323846_go_wp

  call get_command_argument(1, arg); read(arg, *) nx
  call get_command_argument(2, arg); read(arg, *) ny
  call get_command_argument(3, mode)
  call gocean_initialise()
  g = grid_type(GO_ARAKAWA_C, (/GO_BC_EXTERNAL, GO_BC_EXTERNAL, GO_BC_NONE/), GO_OFFSET_NE)
  if (trim(mode) == 'dm') then
     call g%decompose(nx, ny, halo_width=2)
  else
     call g%decompose(nx, ny, halo_width=1)
  end if
  allocate(tmask(g%subdomain%internal%xstop + 1, g%subdomain%internal%ystop + 1))
  do j = 1, size(tmask, 2)
     do i = 1, size(tmask, 1)
        tmask(i, j) = mod(7*i + 13*j + (i*j)/5, 3) - 1
     end do
  end do
  tmask(1:3, 1:3) = 0                 ! a stretch of coast
  call grid_init(g, 1000.0_go_wp, 1000.0_go_wp, tmask)
  prm = momentum_params(20.0_go_wp, 0.00015_go_wp, 50.0_go_wp, 9.80665_go_wp)
  call momentum_coriolis(g, 7.292116e-5_go_wp, pi / 180.0_go_wp)

  do k = 1, NF
     f(k) = r2d_field(g, pts(k))
     call invoke_hash_init(f(k), int(900 + k, c_int64_t))
     call f(k)%read_from_device()
     select case (k)
     case (8, 9, 10); f(k)%data = 10.0_go_wp + f(k)%data
     case (1); f(k)%data = 1000.0_go_wp + f(k)%data                   ! the ring ssha: values no step computes
     case (2, 3, 4, 5); f(k)%data = -7.0_go_wp
     case (6, 7); f(k)%data = 0.4_go_wp * f(k)%data - 0.2_go_wp       ! velocities of both signs
     case default; f(k)%data = 0.05_go_wp * f(k)%data
     end select
     call f(k)%write_to_device()
  end do
  do k = 1, 2
     c_in(k) = r2d_field(g, GO_T_POINTS)
     c_out(k) = r2d_field(g, GO_T_POINTS)
     call invoke_hash_init(c_in(k), int(600 + k, c_int64_t))
     call c_in(k)%read_from_device()
     c_in(k)%data = real(k, go_wp) + c_in(k)%data
     call c_in(k)%write_to_device()
     c_out(k)%data = -7.0_go_wp
     call c_out(k)%write_to_device()
  end do

  if (trim(mode) == 'hw1') then
     call invoke_nemolite_coupled_step_dm(prm, DLESM_TRACER_MUSCL, c_out, c_in, f(1), f(2), f(3), f(4), f(5), f(6), f(7), f(8), &
                                          f(9), f(10), f(11), f(12), f(13))
     call device_sync()
     write(*, '("G: ran where the wrapper must stop")')
     call gocean_finalise()
     stop
  end if

  allocate(before(size(g%tmask, 1), size(g%tmask, 2)))
  before = g%tmask
  call exchange_mask_halos(g)
  if (any(g%tmask /= before)) then
     write(*, '("G: the mask changed")')
  else
     write(*, '("G: the mask is unchanged")')
  end if
  call invoke_nemolite_coupled_step_dm(prm, DLESM_TRACER_HANCOCK, c_out, c_in, f(1), f(2), f(3), f(4), f(5), f(6), f(7), f(8), &
                                       f(9), f(10), f(11), f(12), f(13))
  call device_sync()
  write(*, '("G: extents ",i0," ",i0)') g%nx, g%ny
  do k = 1, 5
     call dump(f(k), names(k))
  end do
  do k = 1, 2
     call dump(c_out(k), names(5 + k))
  end do
  call gocean_finalise()

contains

  subroutine dump(fld, name)
    type(r2d_field), intent(inout), target :: fld
    character(len=*), intent(in) :: name
    type(field_stats_type) :: st
    real(go_wp) :: sum_abs
    sum_abs = field_checksum(fld)
    call field_stats(fld, st)
    write(*, '("G: ",a," checksum ",Z16.16)') trim(name), transfer(sum_abs, 1_c_int64_t)
    write(*, '("G: ",a," stats ",4(Z16.16,1x),i0,1x,i0)') trim(name), transfer(st%min, 1_c_int64_t), &
         transfer(st%max, 1_c_int64_t), transfer(st%sum, 1_c_int64_t), transfer(st%sumsq, 1_c_int64_t), st%count, st%nonfinite
  end subroutine dump

end program ftest_coupled_step
