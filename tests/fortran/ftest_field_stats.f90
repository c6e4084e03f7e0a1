!> GPU test of the Fortran wrappers field_stats / field_locate (tests/test_gpu_fortran_field_stats.py).  One rank: a grid with
!! a land/sea mask that is a function of the cell index; hash-filled T, U and V fields, each shifted to [-0.5, 0.5), with one
!! NaN and one infinity planted in wet cells of the U field and one NaN in a dry cell of the V field.  field_stats of each
!! field without and with the grid's device tmask mirror, field_locate of the first non-finite cell and of the maximum.  The
!! extents, the three internal regions, the mask, the fields, the six stats records and the located cells go to the file
!! OUT (stream access, native byte order).
!!   ftest_field_stats.exe NX NY OUT
program ftest_field_stats
  use iso_c_binding
  use kind_params_mod
  use parallel_mod
  use grid_mod
  use field_mod
  use gocean_mod
  use dlesm_psy_mod
  implicit none
  character(len=256) :: arg, out
  integer :: nx, ny, i, j, k, u, wi, wj, di, dj, loc(2, 12)
  integer, allocatable :: tm(:,:)
  type(grid_type), target :: g
  type(r2d_field), target :: f(3)
  type(field_stats_type) :: st(6)

  call get_command_argument(1, arg); read(arg, *) nx
  call get_command_argument(2, arg); read(arg, *) ny
  call get_command_argument(3, out)
  call gocean_initialise()
  g = grid_type(GO_ARAKAWA_C, (/GO_BC_EXTERNAL, GO_BC_EXTERNAL, GO_BC_NONE/), GO_OFFSET_NE)
  call g%decompose(nx, ny)
  allocate(tm(nx + 2, ny + 2))
  do j = 1, ny + 2
     do i = 1, nx + 2
        tm(i, j) = mod(7*i + 13*j, 3) - 1              ! -1, 0, 1
     end do
  end do
  call grid_init(g, 1.0_go_wp, 1.0_go_wp, tm)
  call grid_to_device(g)
  f(1) = r2d_field(g, GO_T_POINTS)
  f(2) = r2d_field(g, GO_U_POINTS)
  f(3) = r2d_field(g, GO_V_POINTS)
  wi = 0;  wj = 0;  di = 0;  dj = 0
  do k = 1, 3
     call invoke_hash_init(f(k), int(20261017 + k, c_int64_t))
     call f(k)%read_from_device()
     f(k)%data = f(k)%data - 0.5_go_wp
  end do
  ! a wet cell well inside the U field's region for the NaN, the next wet one for the infinity; a dry cell for the V field
  do j = f(2)%internal%ystart + 2, f(2)%internal%ystop
     do i = f(2)%internal%xstart + 1, f(2)%internal%xstop
        if (g%tmask(i, j) > 0 .and. wi == 0) then
           wi = i;  wj = j
        else if (g%tmask(i, j) > 0 .and. di == 0) then
           di = i;  dj = j
        end if
     end do
  end do
  f(2)%data(wi, wj) = ieee_nan()
  f(2)%data(di, dj) = huge(1.0_go_wp)
  f(2)%data(di, dj) = 2.0_go_wp * f(2)%data(di, dj)    ! +inf
  outer: do j = f(3)%internal%ystart, f(3)%internal%ystop
     do i = f(3)%internal%xstart, f(3)%internal%xstop
        if (g%tmask(i, j) <= 0) then
           f(3)%data(i, j) = ieee_nan()
           exit outer
        end if
     end do
  end do outer
  do k = 1, 3
     call f(k)%write_to_device()
  end do

  loc = 0
  do k = 1, 3
     call field_stats(f(k), st(2*k - 1))
     call field_stats(f(k), st(2*k), g%tmask_device)
     call field_locate(f(k), DLESM_LOCATE_NONFINITE, loc(1, 4*k - 3), loc(2, 4*k - 3))
     call field_locate(f(k), DLESM_LOCATE_NONFINITE, loc(1, 4*k - 2), loc(2, 4*k - 2), mask=g%tmask_device)
     call field_locate(f(k), DLESM_LOCATE_EQUAL, loc(1, 4*k - 1), loc(2, 4*k - 1), value=real(st(2*k - 1)%max, go_wp))
     call field_locate(f(k), DLESM_LOCATE_EQUAL, loc(1, 4*k), loc(2, 4*k), value=real(st(2*k)%min, go_wp), mask=g%tmask_device)
  end do

  open(newunit=u, file=trim(out), access='stream', form='unformatted', status='replace')
  write(u) int(g%nx, c_int), int(g%ny, c_int)
  do k = 1, 3
     write(u) int((/f(k)%internal%xstart, f(k)%internal%xstop, f(k)%internal%ystart, f(k)%internal%ystop/), c_int)
  end do
  write(u) int(g%tmask, c_int)
  write(u) f(1)%data, f(2)%data, f(3)%data
  do k = 1, 6
     write(u) st(k)%min, st(k)%max, st(k)%sum, st(k)%sumsq, st(k)%count, st(k)%nonfinite
  end do
  write(u) int(loc, c_int)
  close(u)
  write(*, '("G: stats written, planted (",I0,",",I0,") (",I0,",",I0,")")') wi, wj, di, dj
  call gocean_finalise()
contains
  function ieee_nan() result(x)
    use, intrinsic :: ieee_arithmetic
    real(go_wp) :: x
    x = ieee_value(x, ieee_quiet_nan)
  end function ieee_nan
end program ftest_field_stats
