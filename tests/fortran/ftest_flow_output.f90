!> GPU test of the Fortran wrapper of the model's output fields, flow_output (DESIGN.md section 6.16;
!! tests/test_gpu_fortran_flow_output.py).  A grid with a -1/0/1 user tmask and the level-n fields un, vn, ht, sshn_t from
!! invoke_hash_init (ftest_flow_courant's), six T-point output fields filled with -7; one flow_output that stores all six and
!! two that add them with weight 0.375; prints the array extents and, after the first and after the third call, a hash of
!! the bits of every cell of each output (h = ieor(ishftc(h, 5), bits), cells in memory order), which the test compares with
!! the Python wrapper's arrays on the same inputs.
!!   ftest_flow_output.exe NX NY
program ftest_flow_output
  use iso_c_binding
  use kind_params_mod
  use parallel_mod
  use grid_mod
  use field_mod
  use gocean_mod
  use dlesm_psy_mod
  implicit none
  ! 2 un 3 vn 4 ht 7 sshn_t: ftest_tracer_courant's numbering and seeds
  integer, parameter :: ks(4) = (/2, 3, 4, 7/)
  integer, parameter :: pts(4) = (/GO_U_POINTS, GO_V_POINTS, GO_T_POINTS, GO_T_POINTS/)
  character(len=256) :: arg
  integer :: nx, ny, i, j, k
  integer, allocatable :: tmask(:,:)
  type(grid_type), target :: g
  type(r2d_field), target :: f(4), o(6)

  call get_command_argument(1, arg); read(arg, *) nx
  call get_command_argument(2, arg); read(arg, *) ny
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

  do k = 1, 4
     f(k) = r2d_field(g, pts(k))
     call invoke_hash_init(f(k), int(500 + ks(k), c_int64_t))
     call f(k)%read_from_device()
     select case (ks(k))
     case (2, 3); f(k)%data = 0.4_go_wp * f(k)%data - 0.2_go_wp          ! velocities of both signs
     case (4); f(k)%data = 10.0_go_wp + f(k)%data                       ! depths
     case default; f(k)%data = 0.05_go_wp * f(k)%data                   ! sea-surface heights
     end select
     call f(k)%write_to_device()
  end do
  do k = 1, 6
     o(k) = r2d_field(g, GO_T_POINTS)
     o(k)%data = -7.0_go_wp
     call o(k)%write_to_device()
  end do

  write(*, '("G: extents ",i0," ",i0)') g%nx, g%ny
  call flow_output(f(1), f(2), f(3), f(4), ssh=o(1), ut=o(2), vt=o(3), speed=o(4), ke=o(5), vort=o(6))
  call show('set')
  call flow_output(f(1), f(2), f(3), f(4), o(1), o(2), o(3), o(4), o(5), o(6), 0.375_go_wp)
  call flow_output(f(1), f(2), f(3), f(4), ssh=o(1), ut=o(2), vt=o(3), speed=o(4), ke=o(5), vort=o(6), weight=0.375_go_wp)
  call show('add')
  ! a selection: the velocities alone, stored again over what the sums left
  call flow_output(f(1), f(2), f(3), f(4), ut=o(2), vt=o(3), speed=o(4))
  call show('uvs')
  call gocean_finalise()
contains
  subroutine show(what)
    character(len=*), intent(in) :: what
    integer(c_int64_t) :: h(6)
    integer :: n, a, b
    do n = 1, 6
       call o(n)%read_from_device()
       h(n) = 0_c_int64_t
       do b = lbound(o(n)%data, 2), ubound(o(n)%data, 2)
          do a = lbound(o(n)%data, 1), ubound(o(n)%data, 1)
             h(n) = ieor(ishftc(h(n), 5), transfer(o(n)%data(a, b), 1_c_int64_t))
          end do
       end do
    end do
    write(*, '("G: ",a," hashes ",5(Z16.16,1x),Z16.16)') what, h
  end subroutine show
end program ftest_flow_output
