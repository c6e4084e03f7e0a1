!> GPU test of the Fortran random_walk wrapper (DESIGN.md section 6.22; tests/test_gpu_fortran_random_walk.py).  The grid, the
!! flow and the N particles of ftest_dispersal.f90, and a T-point field kh_t = 5 + 70 * hash(i, j) m2/s from invoke_hash_init.
!! One set takes random_walk with nsub = 3 at tick TICK, is brought into cell order by particle_sort, and takes random_walk
!! with nsub = 2 at tick TICK + 3: the particles keep their random streams through the sort.  After each step the program
!! prints, with the particles brought back into the order of drifters_create through particle_origin, a hash of the bits of
!! px, of py and of status (h = ieor(ishftc(h, 5), bits)) and the number of particles of each status, which the test compares
!! with the restatement; and how many slots the sort moved.
!!   ftest_random_walk.exe N SEED TICK        (SEED and TICK: signed 64-bit decimal numbers)
program ftest_random_walk
  use iso_c_binding
  use kind_params_mod
  use parallel_mod
  use grid_mod
  use field_mod
  use gocean_mod
  use dlesm_psy_mod
  implicit none
  character(len=256) :: arg
  integer :: n, p, nlive
  integer, allocatable :: tmask(:,:), origin(:)
  real(go_wp), allocatable :: px(:), py(:), ox(:), oy(:)
  integer(c_int), allocatable :: st(:), os(:)
  integer(c_long_long) :: seed, tick
  type(grid_type), target :: g
  type(r2d_field), target :: un, vn, kh_t
  type(drifters_type) :: set

  call get_command_argument(1, arg); read(arg, *) n
  call get_command_argument(2, arg); read(arg, *) seed
  call get_command_argument(3, arg); read(arg, *) tick
  call gocean_initialise()
  g = grid_type(GO_ARAKAWA_C, (/GO_BC_EXTERNAL, GO_BC_EXTERNAL, GO_BC_NONE/), GO_OFFSET_NE)
  call g%decompose(23, 19)
  allocate(tmask(g%subdomain%internal%xstop + 1, g%subdomain%internal%ystop + 1))
  tmask = 1
  tmask(24:, :) = -1
  tmask(1, :) = 0;  tmask(:, 1) = 0;  tmask(:, size(tmask, 2)) = 0
  tmask(10:13, 8:11) = 0
  tmask(17, 15) = 0
  call grid_init(g, 1000.0_go_wp, 1000.0_go_wp, tmask)

  un = r2d_field(g, GO_U_POINTS);  vn = r2d_field(g, GO_V_POINTS);  kh_t = r2d_field(g, GO_T_POINTS)
  call invoke_hash_init(un, 617_c_int64_t);  call invoke_hash_init(vn, 618_c_int64_t)
  call invoke_hash_init(kh_t, 622_c_int64_t)
  call un%read_from_device();  call vn%read_from_device();  call kh_t%read_from_device()
  un%data = 3.0_go_wp * un%data - 1.5_go_wp
  vn%data = 3.0_go_wp * vn%data - 1.5_go_wp
  kh_t%data = 5.0_go_wp + 70.0_go_wp * kh_t%data
  call un%write_to_device();  call vn%write_to_device();  call kh_t%write_to_device()

  allocate(px(n), py(n), st(n), ox(n), oy(n), os(n), origin(n))
  do p = 1, n
     px(p) = 0.5_go_wp + 0.125_go_wp * real(mod(37 * (p - 1), 211), go_wp)
     py(p) = 0.5_go_wp + 0.0625_go_wp * real(mod(101 * (p - 1), 353), go_wp)
     st(p) = merge(1 + mod(p, 3), 0, mod(p, 11) == 0)
  end do

  write(*, '("G: extents ",i0," ",i0)') g%nx, g%ny
  call drifters_create(set, px, py, st)
  call random_walk(set, 400.0_go_wp, 3, kh_t, seed, tick, un, vn)
  call show('first')
  call particle_sort(set, un)
  call particle_origin(set, origin, nlive)
  write(*, '("G: sorted nlive ",i0," moved ",i0)') nlive, count(origin /= (/(p, p = 1, n)/))
  call random_walk(set, 400.0_go_wp, 2, kh_t, seed, tick + 3_c_long_long, un, vn)
  call show('second')
  call drifters_free(set)
  call gocean_finalise()
contains
  !> the set as it is now, in the order of drifters_create
  subroutine show(what)
    character(len=*), intent(in) :: what
    integer(c_int64_t) :: h(3)
    integer :: q, cnt(0:3), live
    call drifters_get(set, px, py, st)
    call particle_origin(set, origin, live)
    do q = 1, n
       ox(origin(q)) = px(q);  oy(origin(q)) = py(q);  os(origin(q)) = st(q)
    end do
    h = 0_c_int64_t
    cnt = 0
    do q = 1, n
       h(1) = ieor(ishftc(h(1), 5), transfer(ox(q), 1_c_int64_t))
       h(2) = ieor(ishftc(h(2), 5), transfer(oy(q), 1_c_int64_t))
       h(3) = ieor(ishftc(h(3), 5), int(os(q), c_int64_t))
       cnt(os(q)) = cnt(os(q)) + 1
    end do
    write(*, '("G: ",a," hashes ",2(Z16.16,1x),Z16.16," counts ",3(i0,1x),i0)') what, h, cnt
  end subroutine show
end program ftest_random_walk
