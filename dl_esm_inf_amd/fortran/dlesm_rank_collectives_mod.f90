!> The cross-rank tail of the host-side diagnostics (field_stats, tracer_courant, flow_courant, invoke_jacobi5_residual): the
!! record a device sweep left on this rank made global.  THE one place of this layer that implements the ownership rule of
!! DESIGN.md section 6.14 (`place`).  Every procedure takes the caller's name `who`, stops through gocean_stop with
!! 'who: <dlesm_error_text()>' when a collective fails, and is its own single-rank case: callers need no DIST_MEM_ENABLED guard.
!! No NaN enters these collectives; counts and indices travel as doubles, exact below 2**53.
module rank_collectives_mod
  use iso_c_binding
  use dlesm_hip_mod
  use gocean_mod, only: gocean_stop
  use parallel_utils_mod, only: DIST_MEM_ENABLED, get_rank
  implicit none
  private
  public rank_max, rank_sum, rank_total, place

contains

  !> x becomes the largest x of all ranks (a minimum goes in and comes out negated).
  subroutine rank_max(who, x)
    character(len=*), intent(in) :: who
    real(c_double), intent(inout) :: x
    if (.not. DIST_MEM_ENABLED) return
    if (dlesm_global_max_f64(x) /= 0) call gocean_stop(who // ': ' // dlesm_error_text())
  end subroutine rank_max

  !> x becomes the sum of the x of all ranks.
  subroutine rank_sum(who, x)
    character(len=*), intent(in) :: who
    real(c_double), intent(inout) :: x
    if (.not. DIST_MEM_ENABLED) return
    if (dlesm_global_sum_f64(x) /= 0) call gocean_stop(who // ': ' // dlesm_error_text())
  end subroutine rank_sum

  !> n becomes the total of the n of all ranks.
  subroutine rank_total(who, n)
    character(len=*), intent(in) :: who
    integer(c_int64_t), intent(inout) :: n
    real(c_double) :: x
    x = real(n, c_double)
    call rank_sum(who, x)
    n = nint(x, c_int64_t)
  end subroutine rank_total

  !> top becomes the maximum over the ranks; owner the lowest rank (1-based, get_rank) that attains it -- one that has a cell
  !! (index >= 0) and whose top IS the maximum -- and index that rank's index; index = -1 and owner = 0 when no rank does.
  !! Two maxima and one sum.  On a single rank: owner only.
  subroutine place(who, top, index, owner)
    character(len=*), intent(in) :: who
    real(c_double), intent(inout) :: top
    integer(c_int64_t), intent(inout) :: index
    integer, intent(out) :: owner
    real(c_double) :: x, mine
    logical :: have
    if (.not. DIST_MEM_ENABLED) then
       owner = merge(get_rank(), 0, index >= 0)
       return
    end if
    x = top
    call rank_max(who, x)
    have = index >= 0 .and. top == x
    top = x
    mine = -1.0e9_c_double
    if (have) mine = -real(get_rank(), c_double)
    call rank_max(who, mine)
    owner = 0
    if (mine > -1.0e9_c_double) owner = nint(-mine)
    x = 0.0_c_double
    if (have .and. owner == get_rank()) x = real(index, c_double)
    call rank_sum(who, x)
    index = -1
    if (owner > 0) index = nint(x, c_int64_t)
  end subroutine place

end module rank_collectives_mod
