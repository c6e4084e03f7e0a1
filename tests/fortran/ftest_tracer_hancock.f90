!> GPU test of the Fortran wrappers of time-centred limited tracer transport, invoke_tracer_step_hancock and
!! invoke_tracer_step_hancock_dm (tests/test_gpu_fortran_tracer_hancock.py).
!! Mode "run": a grid with a -1/0/1 user tmask, the nine flow fields and two tracers from invoke_hash_init, one
!! invoke_tracer_step_hancock of both tracers into sentinel-filled outputs; prints the array extents and, per new tracer, the
!! bits of field_checksum and of field_stats without and with the grid's mask, which the test compares with the Python
!! wrapper's on the same inputs.  Mode "dm": the same on a one-rank grid decomposed with halo_width = 2 through
!! invoke_tracer_step_hancock_dm (a plan without messages).  Mode "hw1": invoke_tracer_step_hancock_dm on a halo_width = 1 grid
!! must stop.  Mode "decomposed": invoke_tracer_step_hancock on a grid decomposed into two subdomains must stop.
!!   ftest_tracer_hancock.exe NX NY run|dm|hw1|decomposed
program ftest_tracer_hancock
  use iso_c_binding
  use kind_params_mod
  use parallel_mod
  use grid_mod
  use field_mod
  use gocean_mod
  use dlesm_psy_mod
  implicit none
  ! 1 ssha 2 un 3 vn 4 ht 5 hu 6 hv 7 sshn_t 8 sshn_u 9 sshn_v
  integer, parameter :: pts(9) = (/GO_T_POINTS, GO_U_POINTS, GO_V_POINTS, GO_T_POINTS, GO_U_POINTS, GO_V_POINTS, GO_T_POINTS, &
                                   GO_U_POINTS, GO_V_POINTS/)
  character(len=256) :: arg, mode
  integer :: nx, ny, i, j, k
  integer, allocatable :: tmask(:,:)
  type(grid_type), target :: g
  type(r2d_field), target :: f(9), c_in(2), c_out(2)
  type(field_stats_type) :: st, stm
  real(go_wp) :: sum_abs

  call get_command_argument(1, arg); read(arg, *) nx
  call get_command_argument(2, arg); read(arg, *) ny
  call get_command_argument(3, mode)
  call gocean_initialise()
  g = grid_type(GO_ARAKAWA_C, (/GO_BC_EXTERNAL, GO_BC_EXTERNAL, GO_BC_NONE/), GO_OFFSET_NE)
  if (trim(mode) == 'decomposed') then
     call g%decompose(nx, ny, ndomains=2)
  else if (trim(mode) == 'dm') then
     call g%decompose(nx, ny, halo_width=2)
  else
     call g%decompose(nx, ny)
  end if
  allocate(tmask(g%subdomain%internal%xstop + 1, g%subdomain%internal%ystop + 1))
  do j = 1, size(tmask, 2)
     do i = 1, size(tmask, 1)
        tmask(i, j) = mod(7*i + 13*j + (i*j)/5, 3) - 1
     end do
  end do
  tmask(1:3, 1:3) = 0                 ! a stretch of coast
  call grid_init(g, 1000.0_go_wp, 1000.0_go_wp, tmask)

  do k = 1, 9
     f(k) = r2d_field(g, pts(k))
     call invoke_hash_init(f(k), int(500 + k, c_int64_t))
     call f(k)%read_from_device()
     select case (k)
     case (2, 3); f(k)%data = 0.4_go_wp * f(k)%data - 0.2_go_wp          ! velocities of both signs
     case (4, 5, 6); f(k)%data = 10.0_go_wp + f(k)%data                 ! depths
     case default; f(k)%data = 0.05_go_wp * f(k)%data                   ! sea-surface heights
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

  if (trim(mode) == 'dm' .or. trim(mode) == 'hw1') then
     call invoke_tracer_step_hancock_dm(1.0e7_go_wp, c_out, c_in, f(1), f(2), f(3), f(4), f(5), f(6), f(7), f(8), f(9))
  else
     call invoke_tracer_step_hancock(1.0e7_go_wp, c_out, c_in, f(1), f(2), f(3), f(4), f(5), f(6), f(7), f(8), f(9))
  end if
  call device_sync()
  if (trim(mode) == 'decomposed' .or. trim(mode) == 'hw1') then
     write(*, '("G: ran where the wrapper must stop")')
     call gocean_finalise()
     stop
  end if
  write(*, '("G: extents ",i0," ",i0)') g%nx, g%ny
  do k = 1, 2
     sum_abs = field_checksum(c_out(k))
     call field_stats(c_out(k), st)
     call field_stats(c_out(k), stm, g%tmask_device)
     write(*, '("G: tracer ",i0," checksum ",Z16.16)') k, transfer(sum_abs, 1_c_int64_t)
     write(*, '("G: tracer ",i0," stats ",4(Z16.16,1x),i0,1x,i0)') k, transfer(st%min, 1_c_int64_t), &
          transfer(st%max, 1_c_int64_t), transfer(st%sum, 1_c_int64_t), transfer(st%sumsq, 1_c_int64_t), st%count, st%nonfinite
     write(*, '("G: tracer ",i0," wet stats ",4(Z16.16,1x),i0,1x,i0)') k, transfer(stm%min, 1_c_int64_t), &
          transfer(stm%max, 1_c_int64_t), transfer(stm%sum, 1_c_int64_t), transfer(stm%sumsq, 1_c_int64_t), stm%count, &
          stm%nonfinite
  end do
  call gocean_finalise()
end program ftest_tracer_hancock
