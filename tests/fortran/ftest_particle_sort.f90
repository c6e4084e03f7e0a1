!> GPU test of the Fortran particle-order wrappers (DESIGN.md section 6.18; tests/test_gpu_fortran_particle_sort.py).  The
!! grid, the flow and the N particles of ftest_drifter.f90.  Two sets of the same particles: one is stepped as it is, the
!! other is brought into cell order by particle_sort first.  After drifter_step with nsub = 3 on both, drifters_get and
!! particle_origin of the sorted set must reproduce the unsorted run through origin, bit for bit: slot k of the sorted set
!! holds particle origin(k) of the other.  Prints nlive, a hash of origin (h = ieor(ishftc(h, 5), origin)), which the test
!! compares with the restatement's permutation, the number of slots that moved, and the verdict; then sorts a second time,
!! after which origin must still lead back to the arrays the set was created from.
!!   ftest_particle_sort.exe N
program ftest_particle_sort
  use iso_c_binding
  use kind_params_mod
  use parallel_mod
  use grid_mod
  use field_mod
  use gocean_mod
  use dlesm_psy_mod
  implicit none
  character(len=256) :: arg
  integer :: n, p, k, nlive, moved, bad
  integer, allocatable :: tmask(:,:), origin(:)
  real(go_wp), allocatable :: px(:), py(:), ax(:), ay(:), bx(:), by(:)
  integer(c_int), allocatable :: st(:), as(:), bs(:)
  integer(c_int64_t) :: h
  type(grid_type), target :: g
  type(r2d_field), target :: un, vn
  type(drifters_type) :: plain, sorted

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

  allocate(px(n), py(n), st(n), ax(n), ay(n), as(n), bx(n), by(n), bs(n), origin(n))
  do p = 1, n
     px(p) = 0.5_go_wp + 0.125_go_wp * real(mod(37 * (p - 1), 211), go_wp)
     py(p) = 0.5_go_wp + 0.0625_go_wp * real(mod(101 * (p - 1), 353), go_wp)
     st(p) = merge(1 + mod(p, 3), 0, mod(p, 11) == 0)
  end do

  write(*, '("G: extents ",i0," ",i0)') g%nx, g%ny
  call drifters_create(plain, px, py, st)
  call drifters_create(sorted, px, py, st)
  call particle_origin(sorted, origin, nlive)
  write(*, '("G: before nlive ",i0," identity ",l1)') nlive, all(origin == (/(k, k = 1, n)/))

  call particle_sort(sorted, un)
  call particle_origin(sorted, origin, nlive)
  h = 0_c_int64_t
  moved = 0
  do k = 1, n
     h = ieor(ishftc(h, 5), int(origin(k), c_int64_t))
     if (origin(k) /= k) moved = moved + 1
  end do
  write(*, '("G: sorted nlive ",i0," origin ",Z16.16," moved ",i0)') nlive, h, moved
  call drifters_get(sorted, bx, by, bs)
  write(*, '("G: the sorted set holds the particles it was given ",l1)') same(px, py, st)

  call drifter_step(plain, 400.0_go_wp, 3, un, vn)
  call drifter_step(sorted, 400.0_go_wp, 3, un, vn)
  call drifters_get(plain, ax, ay, as)
  call drifters_get(sorted, bx, by, bs)
  write(*, '("G: the sorted run reproduces the unsorted run ",l1," stepped ",l1)') same(ax, ay, as), any(ax /= px)

  ! a second sort, of the stepped particles: origin still leads back to the arrays of drifters_create
  call particle_sort(sorted, un)
  call particle_origin(sorted, origin, nlive)
  call drifters_get(sorted, bx, by, bs)
  write(*, '("G: after a second sort ",l1," nlive ",i0)') same(ax, ay, as), nlive
  call drifters_free(plain)
  call drifters_free(sorted)
  call gocean_finalise()
contains
  !> slot k of (bx, by, bs) holds element origin(k) of (x, y, s), bit for bit, and origin is a permutation
  logical function same(x, y, s)
    real(go_wp), intent(in) :: x(:), y(:)
    integer(c_int), intent(in) :: s(:)
    integer :: q
    logical, allocatable :: seen(:)
    allocate(seen(n))
    seen = .false.
    bad = 0
    do q = 1, n
       if (origin(q) < 1 .or. origin(q) > n) then
          bad = bad + 1
          cycle
       end if
       seen(origin(q)) = .true.
       if (transfer(bx(q), 1_c_int64_t) /= transfer(x(origin(q)), 1_c_int64_t)) bad = bad + 1
       if (transfer(by(q), 1_c_int64_t) /= transfer(y(origin(q)), 1_c_int64_t)) bad = bad + 1
       if (bs(q) /= s(origin(q))) bad = bad + 1
    end do
    same = bad == 0 .and. all(seen)
  end function same
end program ftest_particle_sort
