!> GPU test of the Fortran cell-bin wrapper (DESIGN.md section 6.19; tests/test_gpu_fortran_cell_bin.py).  The grid and the
!! N particles of ftest_particle_sort.f90.  cell_bin counts the set into a T-point field that was filled with -3: the program
!! prints the sum of the counts over the internal region, a hash of them in row-major order (h = ieor(ishftc(h, 5), count)),
!! which the test compares with the restatement's counts, and whether everything outside the region is still -3.  Then it
!! adds the count twice with alpha = 0.5 and checks the two roundings itself, and counts once more after particle_sort, which
!! must change nothing.
!!   ftest_cell_bin.exe N
program ftest_cell_bin
  use iso_c_binding
  use kind_params_mod
  use parallel_mod
  use grid_mod
  use field_mod
  use gocean_mod
  use dlesm_psy_mod
  implicit none
  character(len=256) :: arg
  integer :: n, p, i, j, total
  integer, allocatable :: tmask(:,:)
  real(go_wp), allocatable :: px(:), py(:), c1(:,:)
  integer(c_int), allocatable :: st(:)
  logical, allocatable :: inside(:,:)
  logical :: ok
  integer(c_int64_t) :: h
  type(grid_type), target :: g
  type(r2d_field), target :: cnt, un
  type(drifters_type) :: set

  call get_command_argument(1, arg); read(arg, *) n
  call gocean_initialise()
  g = grid_type(GO_ARAKAWA_C, (/GO_BC_EXTERNAL, GO_BC_EXTERNAL, GO_BC_NONE/), GO_OFFSET_NE)
  call g%decompose(23, 19)
  allocate(tmask(g%subdomain%internal%xstop + 1, g%subdomain%internal%ystop + 1))
  tmask = 1
  tmask(24:, :) = -1
  tmask(1, :) = 0;  tmask(:, 1) = 0;  tmask(:, size(tmask, 2)) = 0
  call grid_init(g, 1000.0_go_wp, 1000.0_go_wp, tmask)

  cnt = r2d_field(g, GO_T_POINTS);  un = r2d_field(g, GO_U_POINTS)
  cnt%data = -3.0_go_wp
  call cnt%write_to_device()
  allocate(px(n), py(n), st(n), c1(g%nx, g%ny), inside(g%nx, g%ny))
  do p = 1, n
     px(p) = 0.5_go_wp + 0.125_go_wp * real(mod(37 * (p - 1), 211), go_wp)
     py(p) = 0.5_go_wp + 0.0625_go_wp * real(mod(101 * (p - 1), 353), go_wp)
     st(p) = merge(1 + mod(p, 3), 0, mod(p, 11) == 0)
  end do
  inside = .false.
  inside(cnt%internal%xstart:cnt%internal%xstop, cnt%internal%ystart:cnt%internal%ystop) = .true.

  write(*, '("G: extents ",i0," ",i0," region ",i0," ",i0," ",i0," ",i0)') g%nx, g%ny, cnt%internal%xstart, &
       cnt%internal%xstop, cnt%internal%ystart, cnt%internal%ystop
  call drifters_create(set, px, py, st)
  call cell_bin(set, cnt)
  call cnt%read_from_device()
  c1 = cnt%data(1:g%nx, 1:g%ny)
  h = 0_c_int64_t
  total = 0
  do j = cnt%internal%ystart, cnt%internal%ystop
     do i = cnt%internal%xstart, cnt%internal%xstop
        h = ieor(ishftc(h, 5), int(c1(i, j), c_int64_t))
        total = total + int(c1(i, j))
     end do
  end do
  write(*, '("G: count sum ",i0," hash ",Z16.16," outside ",l1)') total, h, all(inside .or. c1 == -3.0_go_wp)

  call cell_bin(set, cnt, 1, 0.5_go_wp)
  call cell_bin(set, cnt, mode=1, alpha=0.5_go_wp)
  call cnt%read_from_device()
  ok = .true.
  do j = 1, g%ny
     do i = 1, g%nx
        if (inside(i, j) .and. c1(i, j) > 0.0_go_wp) then
           ok = ok .and. cnt%data(i, j) == (c1(i, j) + 0.5_go_wp * c1(i, j)) + 0.5_go_wp * c1(i, j)
        else
           ok = ok .and. cnt%data(i, j) == c1(i, j)
        end if
     end do
  end do
  write(*, '("G: added twice ",l1)') ok

  call particle_sort(set, un)
  call cell_bin(set, cnt, alpha=1.0_go_wp)
  call cnt%read_from_device()
  write(*, '("G: the same after a sort ",l1)') all(cnt%data(1:g%nx, 1:g%ny) == c1)
  call drifters_free(set)
  call gocean_finalise()
end program ftest_cell_bin
