!> GPU test of the Fortran wrappers of the open-boundary kernels (tests/test_gpu_fortran_open_bc.py).
!! Mode "run": a channel -- open (-1) first and last internal columns, an open row along the south, land to the north --
!! then invoke_bc_ssh, invoke_bc_flather_u and invoke_bc_flather_v on one set of outputs and invoke_bc_open on a second.
!! Extents, the internal regions, tmask, ssh_bc, the inputs and both sets of outputs go to the file OUT (stream access,
!! native byte order).  Mode "refuse": a channel one cell wide between two open columns; a wrapper must stop.
!!   ftest_open_bc.exe NX NY run|refuse OUT
program ftest_open_bc
  use iso_c_binding
  use kind_params_mod
  use parallel_mod
  use grid_mod
  use field_mod
  use gocean_mod
  use dlesm_psy_mod
  implicit none
  character(len=256) :: arg, mode, out
  integer :: nx, ny, i, j, k, u, xs, xe, ys, ye
  integer, allocatable :: tmask(:,:)
  type(grid_type), target :: g
  type(r2d_field), target :: f(5), o(6)
  type(c_momentum_params) :: prm
  real(go_wp) :: ssh_bc
  real(go_wp), parameter :: pi = 3.14159265358979323846_go_wp

  call get_command_argument(1, arg); read(arg, *) nx
  call get_command_argument(2, arg); read(arg, *) ny
  call get_command_argument(3, mode)
  call get_command_argument(4, out)
  call gocean_initialise()
  g = grid_type(GO_ARAKAWA_C, (/GO_BC_EXTERNAL, GO_BC_EXTERNAL, GO_BC_NONE/), GO_OFFSET_NE)
  call g%decompose(nx, ny)
  xs = g%subdomain%internal%xstart;  xe = g%subdomain%internal%xstop
  ys = g%subdomain%internal%ystart;  ye = g%subdomain%internal%ystop
  allocate(tmask(xe + 1, ye + 1))
  tmask = 1
  tmask(xs - 1, :) = 0;  tmask(xe + 1, :) = 0
  tmask(:, ye) = 0;  tmask(:, ye + 1) = 0          ! land to the north
  if (trim(mode) == 'refuse') then
     tmask(xs + 3, :) = -1;  tmask(xs + 5, :) = -1  ! one wet column between two open ones
  else
     tmask(xs, ys:ye - 1) = -1;  tmask(xe, ys:ye - 1) = -1
     tmask(xs + 1:xe - 1, ys) = -1                  ! an open row along the south
     tmask(xs + 1:xe - 1, ys - 1) = 0
  end if
  call grid_init(g, 1000.0_go_wp, 1000.0_go_wp, tmask)
  prm = momentum_params(20.0_go_wp, 0.00015_go_wp, 50.0_go_wp, 9.80665_go_wp)
  ssh_bc = tide_ssh(0.1_go_wp, 2.0_go_wp * pi / 43200.0_go_wp, 1500.0_go_wp)

  ! hu, sshn_u, hv, sshn_v, sshn_t
  do k = 1, 5
     select case (k)
     case (1, 2); f(k) = r2d_field(g, GO_U_POINTS)
     case (3, 4); f(k) = r2d_field(g, GO_V_POINTS)
     case default; f(k) = r2d_field(g, GO_T_POINTS)
     end select
     call invoke_hash_init(f(k), int(700 + k, c_int64_t))
     call f(k)%read_from_device()
     if (k == 1 .or. k == 3) then
        f(k)%data = 5.0_go_wp + 10.0_go_wp * f(k)%data
     else
        f(k)%data = 0.1_go_wp * f(k)%data - 0.05_go_wp
     end if
     call f(k)%write_to_device()
  end do
  ! ssha, ua, va twice: ssha sentinel-filled, ua / va with values of their own
  do k = 1, 6
     select case (mod(k - 1, 3))
     case (0); o(k) = r2d_field(g, GO_T_POINTS)
     case (1); o(k) = r2d_field(g, GO_U_POINTS)
     case default; o(k) = r2d_field(g, GO_V_POINTS)
     end select
     if (mod(k - 1, 3) == 0) then
        o(k)%data = -7.0_go_wp
     else
        do j = 1, g%ny
           do i = 1, g%nx
              o(k)%data(i, j) = 0.001_go_wp * real(mod(13*i + 7*j, 101) - 50, go_wp)
           end do
        end do
     end if
     call o(k)%write_to_device()
  end do

  call invoke_bc_ssh(o(1), ssh_bc)
  if (trim(mode) == 'refuse') then
     call device_sync()
     write(*, '("G: refused mask ran")')
     call gocean_finalise()
     stop
  end if
  call invoke_bc_flather_u(prm, o(2), f(1), f(2), f(5))
  call invoke_bc_flather_v(prm, o(3), f(3), f(4), f(5))
  call invoke_bc_open(prm, ssh_bc, o(4), o(5), o(6), f(1), f(2), f(3), f(4), f(5))
  call device_sync()
  do k = 1, 6
     call o(k)%read_from_device()
  end do

  open(newunit=u, file=trim(out), access='stream', form='unformatted', status='replace')
  write(u) int(g%nx, c_int), int(g%ny, c_int)
  write(u) int((/o(1)%internal%xstart, o(1)%internal%xstop, o(1)%internal%ystart, o(1)%internal%ystop/), c_int)
  write(u) int((/o(2)%internal%xstart, o(2)%internal%xstop, o(2)%internal%ystart, o(2)%internal%ystop/), c_int)
  write(u) int((/o(3)%internal%xstart, o(3)%internal%xstop, o(3)%internal%ystart, o(3)%internal%ystop/), c_int)
  write(u) int(g%tmask, c_int)
  write(u) real(ssh_bc, c_double)
  do k = 1, 5
     write(u) f(k)%data
  end do
  do k = 1, 6
     write(u) o(k)%data
  end do
  close(u)
  write(*, '("G: wrote ",a)') trim(out)
  call gocean_finalise()

end program ftest_open_bc
