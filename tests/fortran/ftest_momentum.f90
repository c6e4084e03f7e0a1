!> GPU test of the Fortran wrappers of the NEMOLite2D-class momentum and next_ssh kernels (tests/test_gpu_fortran_momentum.py).
!! Mode "run": a grid with a -1/0/1 user tmask, momentum_coriolis, then invoke_next_sshu / invoke_next_sshv,
!! invoke_momentum_u + invoke_momentum_v (separate) and invoke_momentum (fused) on sentinel-filled outputs.  Everything the
!! checker needs -- extents, internal regions, the grid arrays, the host-computed fcor_u / fcor_v, the inputs and the
!! outputs -- goes to the file OUT (stream access, native byte order).  Mode "nocor": a momentum wrapper without
!! momentum_coriolis must stop.
!!   ftest_momentum.exe NX NY run|nocor OUT
program ftest_momentum
  use iso_c_binding
  use kind_params_mod
  use parallel_mod
  use grid_mod
  use field_mod
  use gocean_mod
  use dlesm_psy_mod
  implicit none
  character(len=256) :: arg, mode, out
  integer :: nx, ny, i, j, k, u
  integer, allocatable :: tmask(:,:)
  type(grid_type), target :: g
  type(r2d_field), target :: f(10), ua, va, ua2, va2, sshu, sshv
  type(c_momentum_params) :: prm
  real(go_wp), parameter :: pi = 3.14159265358979323846_go_wp

  call get_command_argument(1, arg); read(arg, *) nx
  call get_command_argument(2, arg); read(arg, *) ny
  call get_command_argument(3, mode)
  call get_command_argument(4, out)
  call gocean_initialise()
  g = grid_type(GO_ARAKAWA_C, (/GO_BC_EXTERNAL, GO_BC_EXTERNAL, GO_BC_NONE/), GO_OFFSET_NE)
  call g%decompose(nx, ny)
  allocate(tmask(g%subdomain%internal%xstop + 1, g%subdomain%internal%ystop + 1))
  do j = 1, size(tmask, 2)
     do i = 1, size(tmask, 1)
        tmask(i, j) = mod(7*i + 13*j + (i*j)/5, 3) - 1
     end do
  end do
  tmask(1:3, 1:3) = 0                 ! a stretch of coast
  call grid_init(g, 1000.0_go_wp, 1000.0_go_wp, tmask)
  prm = momentum_params(20.0_go_wp, 0.00015_go_wp, 50.0_go_wp, 9.80665_go_wp)

  ! un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, ssha_v
  do k = 1, 10
     select case (k)
     case (1, 5, 6, 9); f(k) = r2d_field(g, GO_U_POINTS)
     case (2, 7, 8, 10); f(k) = r2d_field(g, GO_V_POINTS)
     case default; f(k) = r2d_field(g, GO_T_POINTS)
     end select
     call invoke_hash_init(f(k), int(500 + k, c_int64_t))
     call f(k)%read_from_device()
     select case (k)
     case (1, 2)                      ! velocities of both signs, with +0.0 and -0.0 among them
        f(k)%data = 0.4_go_wp * f(k)%data - 0.2_go_wp
        do j = 1, g%ny
           do i = 1, g%nx
              if (mod(i + 2*j, 7) == 0) f(k)%data(i, j) = 0.0_go_wp
              if (mod(2*i + j, 11) == 0) f(k)%data(i, j) = -0.0_go_wp
           end do
        end do
     case (3, 5, 7)                   ! depths
        f(k)%data = 10.0_go_wp + f(k)%data
     case default                     ! sea-surface heights
        f(k)%data = 0.05_go_wp * f(k)%data
     end select
     call f(k)%write_to_device()
  end do
  ua = r2d_field(g, GO_U_POINTS);  va = r2d_field(g, GO_V_POINTS)
  ua2 = r2d_field(g, GO_U_POINTS);  va2 = r2d_field(g, GO_V_POINTS)
  sshu = r2d_field(g, GO_U_POINTS);  sshv = r2d_field(g, GO_V_POINTS)
  call fill(ua);  call fill(va);  call fill(ua2);  call fill(va2);  call fill(sshu);  call fill(sshv)

  if (trim(mode) == 'nocor') then
     call invoke_momentum_u(prm, ua, f(1), f(2), f(3), f(4), f(5), f(6), f(7), f(8), f(9))
     call device_sync()
     write(*, '("G: momentum without coriolis ran")')
     call gocean_finalise()
     stop
  end if

  call momentum_coriolis(g, 7.292116e-5_go_wp, pi / 180.0_go_wp)
  call invoke_next_sshu(sshu, f(4))
  call invoke_next_sshv(sshv, f(4))
  call invoke_momentum_u(prm, ua, f(1), f(2), f(3), f(4), f(5), f(6), f(7), f(8), f(9))
  call invoke_momentum_v(prm, va, f(1), f(2), f(3), f(4), f(5), f(6), f(7), f(8), f(10))
  call invoke_momentum(prm, ua2, va2, f(1), f(2), f(3), f(4), f(5), f(6), f(7), f(8), f(9), f(10))
  call device_sync()
  call ua%read_from_device();  call va%read_from_device()
  call ua2%read_from_device();  call va2%read_from_device()
  call sshu%read_from_device();  call sshv%read_from_device()

  open(newunit=u, file=trim(out), access='stream', form='unformatted', status='replace')
  write(u) int(g%nx, c_int), int(g%ny, c_int)
  write(u) int((/ua%internal%xstart, ua%internal%xstop, ua%internal%ystart, ua%internal%ystop/), c_int)
  write(u) int((/va%internal%xstart, va%internal%xstop, va%internal%ystart, va%internal%ystop/), c_int)
  write(u) int(g%tmask, c_int)
  write(u) g%dx_t, g%dy_t, g%dx_u, g%dy_u, g%dx_v, g%dy_v, g%area_t, g%area_u, g%area_v, g%fcor_u, g%fcor_v
  do k = 1, 10
     write(u) f(k)%data
  end do
  write(u) ua%data, va%data, ua2%data, va2%data, sshu%data, sshv%data
  close(u)
  write(*, '("G: wrote ",a)') trim(out)
  call gocean_finalise()

contains

  subroutine fill(fld)
    type(r2d_field), intent(inout), target :: fld
    fld%data = -7.0_go_wp
    call fld%write_to_device()
  end subroutine fill

end program ftest_momentum
