!> GPU test of the Fortran wrapper of the tracer schemes' Courant check, tracer_courant (DESIGN.md section 6.14;
!! tests/test_gpu_fortran_tracer_courant.py).  A grid with a -1/0/1 user tmask and the eight level-n flow fields from
!! invoke_hash_init (ftest_tracer_hancock's), one tracer_courant with the default limits and one with limits of 1 and 2 and the
!! owning ranks asked for; prints the array extents and, per call, the bits of the two maxima and the six integers of the
!! record, which the test compares with the Python wrapper's on the same inputs.
!!   ftest_tracer_courant.exe NX NY RDT
program ftest_tracer_courant
  use iso_c_binding
  use kind_params_mod
  use parallel_mod
  use grid_mod
  use field_mod
  use gocean_mod
  use dlesm_psy_mod
  implicit none
  ! 2 un 3 vn 4 ht 5 hu 6 hv 7 sshn_t 8 sshn_u 9 sshn_v (1 is ftest_tracer_hancock's ssha, which this check does not read)
  integer, parameter :: pts(9) = (/GO_T_POINTS, GO_U_POINTS, GO_V_POINTS, GO_T_POINTS, GO_U_POINTS, GO_V_POINTS, GO_T_POINTS, &
                                   GO_U_POINTS, GO_V_POINTS/)
  character(len=256) :: arg
  integer :: nx, ny, i, j, k, face_rank, outflow_rank
  integer, allocatable :: tmask(:,:)
  type(grid_type), target :: g
  type(r2d_field), target :: f(9)
  type(tracer_courant_type) :: res
  real(go_wp) :: rdt

  call get_command_argument(1, arg); read(arg, *) nx
  call get_command_argument(2, arg); read(arg, *) ny
  call get_command_argument(3, arg); read(arg, *) rdt
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

  do k = 2, 9
     f(k) = r2d_field(g, pts(k))
     call invoke_hash_init(f(k), int(500 + k, c_int64_t))
     call f(k)%read_from_device()
     select case (k)
     case (2, 3); f(k)%data = 0.4_go_wp * f(k)%data - 0.2_go_wp          ! velocities of both signs
     case (4, 5, 6); f(k)%data = 10.0_go_wp + f(k)%data                 ! depths
     case default; f(k)%data = 0.05_go_wp * f(k)%data                   ! sea-surface heights
     end select
     call f(k)%write_to_device()
  end do

  write(*, '("G: extents ",i0," ",i0)') g%nx, g%ny
  call tracer_courant(rdt, f(2), f(3), f(4), f(5), f(6), f(7), f(8), f(9), res)
  call show('default')
  face_rank = -5;  outflow_rank = -5
  call tracer_courant(rdt, f(2), f(3), f(4), f(5), f(6), f(7), f(8), f(9), res, face_limit=1.0_go_wp, &
                      outflow_limit=2.0_go_wp, face_rank=face_rank, outflow_rank=outflow_rank)
  call show('limits 1 2')
  write(*, '("G: ranks ",i0," ",i0)') face_rank, outflow_rank
  call gocean_finalise()
contains
  subroutine show(what)
    character(len=*), intent(in) :: what
    write(*, '("G: ",a," record ",2(Z16.16,1x),5(i0,1x),i0)') what, transfer(res%face_max, 1_c_int64_t), &
         transfer(res%outflow_max, 1_c_int64_t), res%face_index, res%outflow_index, res%face_over, res%outflow_over, &
         res%invalid, res%wet
  end subroutine show
end program ftest_tracer_courant
