!> GPU test of the Fortran drifter wrappers (DESIGN.md section 6.17; tests/test_gpu_fortran_drifter.py).  The 26 x 22 grid
!! of tests/drifter_cases.py as grid_init makes it from a 23 x 19 domain: land on the west, south and north, open columns
!! from 24 eastwards, the 4 x 4 island and the rock; un and vn from invoke_hash_init, scaled to +-1.5 m/s.  N particles at
!! positions that are exact binary fractions, every eleventh one not ACTIVE; drifters_create, one drifter_step with nsub = 1,
!! one with nsub = 3, drifters_get after each; prints the array extents and, after each call, a hash of the bits of px, of
!! py and of status (h = ieor(ishftc(h, 5), bits)) and the number of particles of each status, which the test compares with
!! the Python wrapper's arrays on the same inputs.
!!   ftest_drifter.exe N
program ftest_drifter
  use iso_c_binding
  use kind_params_mod
  use parallel_mod
  use grid_mod
  use field_mod
  use gocean_mod
  use dlesm_psy_mod
  implicit none
  character(len=256) :: arg
  integer :: n, i, j, p
  integer, allocatable :: tmask(:,:)
  real(go_wp), allocatable :: px(:), py(:)
  integer(c_int), allocatable :: st(:)
  type(grid_type), target :: g
  type(r2d_field), target :: un, vn
  type(drifters_type) :: set

  call get_command_argument(1, arg); read(arg, *) n
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

  un = r2d_field(g, GO_U_POINTS);  vn = r2d_field(g, GO_V_POINTS)
  call invoke_hash_init(un, 617_c_int64_t);  call invoke_hash_init(vn, 618_c_int64_t)
  call un%read_from_device();  call vn%read_from_device()
  un%data = 3.0_go_wp * un%data - 1.5_go_wp
  vn%data = 3.0_go_wp * vn%data - 1.5_go_wp
  call un%write_to_device();  call vn%write_to_device()

  allocate(px(n), py(n), st(n))
  do p = 1, n
     px(p) = 0.5_go_wp + 0.125_go_wp * real(mod(37 * (p - 1), 211), go_wp)
     py(p) = 0.5_go_wp + 0.0625_go_wp * real(mod(101 * (p - 1), 353), go_wp)
     st(p) = merge(1 + mod(p, 3), 0, mod(p, 11) == 0)
  end do

  write(*, '("G: extents ",i0," ",i0)') g%nx, g%ny
  call drifters_create(set, px, py, st)
  call drifter_step(set, 400.0_go_wp, 1, un, vn)
  call drifters_get(set, px, py, st)
  call show('one')
  call drifter_step(set, 400.0_go_wp, 3, un, vn)
  call drifters_get(set, px, py, st)
  call show('three')
  ! a set without a status array: all ACTIVE
  call drifters_create(set, px, py)
  call drifter_step(set, 400.0_go_wp, 2, un, vn)
  call drifters_get(set, px, py, st)
  call show('again')
  call drifters_free(set)
  call gocean_finalise()
contains
  subroutine show(what)
    character(len=*), intent(in) :: what
    integer(c_int64_t) :: h(3)
    integer :: q, cnt(0:3)
    h = 0_c_int64_t
    cnt = 0
    do q = 1, n
       h(1) = ieor(ishftc(h(1), 5), transfer(px(q), 1_c_int64_t))
       h(2) = ieor(ishftc(h(2), 5), transfer(py(q), 1_c_int64_t))
       h(3) = ieor(ishftc(h(3), 5), int(st(q), c_int64_t))
       cnt(st(q)) = cnt(st(q)) + 1
    end do
    write(*, '("G: ",a," hashes ",2(Z16.16,1x),Z16.16," counts ",3(i0,1x),i0)') what, h, cnt
  end subroutine show
end program ftest_drifter
