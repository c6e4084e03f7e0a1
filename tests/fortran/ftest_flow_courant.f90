!> GPU test of the Fortran wrapper of the flow step's stability check, flow_courant (DESIGN.md section 6.15;
!! tests/test_gpu_fortran_flow_courant.py).  A grid with a -1/0/1 user tmask and the level-n fields un, vn, ht, sshn_t from
!! invoke_hash_init (ftest_tracer_courant's), one flow_courant with g and visc given and the default limits and one with four
!! limits and the owning ranks asked for; prints the array extents and, per call, the bits of the four doubles and the ten
!! integers of the record, which the test compares with the Python wrapper's on the same inputs.
!!   ftest_flow_courant.exe NX NY RDT VISC
program ftest_flow_courant
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
  integer :: nx, ny, i, j, k, ranks(4)
  integer, allocatable :: tmask(:,:)
  type(grid_type), target :: g
  type(r2d_field), target :: f(4)
  type(flow_courant_type) :: res
  real(go_wp) :: rdt, visc

  call get_command_argument(1, arg); read(arg, *) nx
  call get_command_argument(2, arg); read(arg, *) ny
  call get_command_argument(3, arg); read(arg, *) rdt
  call get_command_argument(4, arg); read(arg, *) visc
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

  write(*, '("G: extents ",i0," ",i0)') g%nx, g%ny
  call flow_courant(rdt, f(1), f(2), f(3), f(4), res, g=9.80665_go_wp, visc=visc)
  call show('default')
  ranks = -5
  call flow_courant(rdt, f(1), f(2), f(3), f(4), res, g=9.80665_go_wp, visc=visc, gravity_limit=1.0_go_wp, &
                    advective_limit=0.015_go_wp, viscous_limit=0.0125_go_wp, depth_limit=10.5_go_wp, gravity_rank=ranks(1), &
                    advective_rank=ranks(2), viscous_rank=ranks(3), depth_rank=ranks(4))
  call show('limits')
  write(*, '("G: ranks ",3(i0,1x),i0)') ranks
  call gocean_finalise()
contains
  subroutine show(what)
    character(len=*), intent(in) :: what
    write(*, '("G: ",a," record ",4(Z16.16,1x),11(i0,1x),i0)') what, transfer(res%gravity_max, 1_c_int64_t), &
         transfer(res%advective_max, 1_c_int64_t), transfer(res%viscous_max, 1_c_int64_t), &
         transfer(res%depth_min, 1_c_int64_t), res%gravity_index, res%advective_index, res%viscous_index, res%depth_index, &
         res%gravity_over, res%advective_over, res%viscous_over, res%shallow, res%invalid, res%wet, res%reserved
  end subroutine show
end program ftest_flow_courant
