!> rank_collectives_mod between processes: no kernel, no field -- gocean_initialise, then place and rank_total on inputs that
!! are functions of get_rank().  Every rank prints the same lines (tests/test_a_fortran_rank_collectives_gpu.py holds the
!! closed forms): per case the top as 16 hex digits, the owner and the index; then the two totals.
program ftest_rank_collectives
  use iso_c_binding
  use parallel_mod
  use gocean_mod
  use rank_collectives_mod
  implicit none
  integer :: r
  integer(c_int64_t) :: cell, nocell, n
  real(c_double) :: x

  call gocean_initialise()
  r = get_rank()
  cell = 100 + r                                   ! this rank's cell: another index on every rank
  nocell = -1

  call show('tie', 2.5_c_double, cell)                                      ! all ranks tie, all hold a cell
  call show('distinct', 0.25_c_double * r, int(7 * r, c_int64_t))           ! the last rank holds the largest
  call show('tie-1-empty', 2.5_c_double, merge(nocell, cell, r == 1))       ! a tie, but rank 1 holds no cell
  call show('nobody', 0.0_c_double, nocell)
  call show('negated', -(10.0_c_double + r), cell)                          ! a minimum 10 + r as the maximum of its negative
  call show('lower-top', merge(1.0_c_double, 3.0_c_double, r == 1), cell)   ! rank 1 has a cell, but not the top

  n = r
  call rank_total('ftest_rank_collectives', n)
  write(*, '("C: total small ",I0)') n
  n = 2_c_int64_t**40 + r
  call rank_total('ftest_rank_collectives', n)
  write(*, '("C: total large ",I0)') n
  x = 0.5_c_double * r
  call rank_sum('ftest_rank_collectives', x)
  write(*, '("C: sum ",Z16.16)') transfer(x, 0_c_int64_t)
  x = -1.5_c_double * r
  call rank_max('ftest_rank_collectives', x)
  write(*, '("C: max ",Z16.16)') transfer(x, 0_c_int64_t)
  call gocean_finalise()

contains

  subroutine show(name, local_top, local_index)
    character(len=*), intent(in) :: name
    real(c_double), intent(in) :: local_top
    integer(c_int64_t), intent(in) :: local_index
    real(c_double) :: top
    integer(c_int64_t) :: index
    integer :: owner
    top = local_top;  index = local_index
    call place('ftest_rank_collectives', top, index, owner)
    write(*, '("C: ",A," top ",Z16.16," owner ",I0," index ",I0)') name, transfer(top, 0_c_int64_t), owner, index
  end subroutine show

end program ftest_rank_collectives
