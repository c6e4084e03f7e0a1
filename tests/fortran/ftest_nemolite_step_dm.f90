!> GPU test of the Fortran wrapper of the one-call NEMOLite2D-class step on a decomposed grid, invoke_nemolite_step_dm
!! (tests/test_gpu_fortran_nemolite_step_dm.py).  Mode "run": on one rank (the wrapper hands the C entry a plan without
!! messages) a channel -- open (-1) first and last internal columns, land rows north and south, an island -- with
!! momentum_coriolis; two sets of fields from the same start, three tidal steps each, rotating by reference: set A through
!! invoke_nemolite_step, set B through invoke_nemolite_step_dm; then one closed-basin step of each.  Prints, per step and
!! array, whether the two sets hold the same bits.  Mode "nocoriolis": invoke_nemolite_step_dm before momentum_coriolis must
!! stop.  Mode "hw2": the same call on a grid decomposed with halo_width = 2 must stop.
!!   ftest_nemolite_step_dm.exe NX NY run|nocoriolis|hw2
program ftest_nemolite_step_dm
  use iso_c_binding
  use kind_params_mod
  use parallel_mod
  use grid_mod
  use field_mod
  use gocean_mod
  use dlesm_psy_mod
  implicit none
  integer, parameter :: NF = 13
  ! 1 ssha 2 ssha_u 3 ssha_v 4 ua 5 va 6 un 7 vn 8 ht 9 hu 10 hv 11 sshn_t 12 sshn_u 13 sshn_v
  integer, parameter :: pts(NF) = (/GO_T_POINTS, GO_U_POINTS, GO_V_POINTS, GO_U_POINTS, GO_V_POINTS, GO_U_POINTS, &
                                    GO_V_POINTS, GO_T_POINTS, GO_U_POINTS, GO_V_POINTS, GO_T_POINTS, GO_U_POINTS, GO_V_POINTS/)
  character(len=8), parameter :: names(NF) = (/'ssha    ', 'ssha_u  ', 'ssha_v  ', 'ua      ', 'va      ', 'un      ', &
                                               'vn      ', 'ht      ', 'hu      ', 'hv      ', 'sshn_t  ', 'sshn_u  ', &
                                               'sshn_v  '/)
  character(len=256) :: arg, mode
  integer :: nx, ny, k, step, xs, xe, ys, ye, ndiff
  integer :: ia(NF), ib(NF)
  integer, allocatable :: tmask(:,:)
  type(grid_type), target :: g
  type(r2d_field), target :: a(NF), b(NF)
  type(c_momentum_params) :: prm
  real(go_wp) :: ssh_bc
  real(go_wp), parameter :: pi = 3.14159265358979323846_go_wp

  call get_command_argument(1, arg); read(arg, *) nx
  call get_command_argument(2, arg); read(arg, *) ny
  call get_command_argument(3, mode)
  call gocean_initialise()
  g = grid_type(GO_ARAKAWA_C, (/GO_BC_EXTERNAL, GO_BC_EXTERNAL, GO_BC_NONE/), GO_OFFSET_NE)
  if (trim(mode) == 'hw2') then
     call g%decompose(nx, ny, halo_width=2)
  else
     call g%decompose(nx, ny, halo_width=1)
  end if
  xs = g%subdomain%internal%xstart;  xe = g%subdomain%internal%xstop
  ys = g%subdomain%internal%ystart;  ye = g%subdomain%internal%ystop
  allocate(tmask(xe + 1, ye + 1))
  tmask = 1
  tmask(xs - 1, :) = 0;  tmask(xe + 1, :) = 0
  tmask(:, ys - 1) = 0;  tmask(:, ys) = 0;  tmask(:, ye) = 0;  tmask(:, ye + 1) = 0
  tmask(xs, ys + 1:ye - 1) = -1;  tmask(xe, ys + 1:ye - 1) = -1
  tmask(xs + nx / 3:xs + nx / 3 + 4, ys + ny / 3:ys + ny / 3 + 3) = 0     ! an island
  call grid_init(g, 1000.0_go_wp, 1000.0_go_wp, tmask)
  prm = momentum_params(20.0_go_wp, 0.00015_go_wp, 50.0_go_wp, 9.80665_go_wp)

  do k = 1, NF
     a(k) = r2d_field(g, pts(k))
     b(k) = r2d_field(g, pts(k))
     call invoke_hash_init(a(k), int(900 + k, c_int64_t))
     call a(k)%read_from_device()
     select case (k)
     case (8, 9, 10); a(k)%data = 10.0_go_wp + a(k)%data
     case (1); a(k)%data = 1000.0_go_wp + a(k)%data                   ! the ring ssha: values no step computes
     case (2, 3, 4, 5); a(k)%data = -7.0_go_wp
     case default; a(k)%data = 0.01_go_wp * (a(k)%data - 0.5_go_wp)
     end select
     b(k)%data = a(k)%data
     call a(k)%write_to_device()
     call b(k)%write_to_device()
     ia(k) = k;  ib(k) = k
  end do

  if (trim(mode) == 'nocoriolis') then
     call invoke_nemolite_step_dm(prm, b(1), b(2), b(3), b(4), b(5), b(6), b(7), b(8), b(9), b(10), b(11), b(12), b(13))
     call device_sync()
     write(*, '("G: ran without coriolis")')
     call gocean_finalise()
     stop
  end if
  call momentum_coriolis(g, 7.292116e-5_go_wp, pi / 180.0_go_wp)
  if (trim(mode) == 'hw2') then
     call invoke_nemolite_step_dm(prm, b(1), b(2), b(3), b(4), b(5), b(6), b(7), b(8), b(9), b(10), b(11), b(12), b(13))
     call device_sync()
     write(*, '("G: ran on halo_width 2")')
     call gocean_finalise()
     stop
  end if

  ndiff = 0
  do step = 1, 4
     if (step <= 3) then
        ssh_bc = tide_ssh(0.1_go_wp, 2.0_go_wp * pi / 43200.0_go_wp, 20.0_go_wp * step)
        call sequence(.true.)
        call invoke_nemolite_step_dm(prm, b(ib(1)), b(ib(2)), b(ib(3)), b(ib(4)), b(ib(5)), b(ib(6)), b(ib(7)), &
                                     b(ib(8)), b(ib(9)), b(ib(10)), b(ib(11)), b(ib(12)), b(ib(13)), ssh_bc)
     else
        call sequence(.false.)
        call invoke_nemolite_step_dm(prm, b(ib(1)), b(ib(2)), b(ib(3)), b(ib(4)), b(ib(5)), b(ib(6)), b(ib(7)), &
                                     b(ib(8)), b(ib(9)), b(ib(10)), b(ib(11)), b(ib(12)), b(ib(13)))
     end if
     call device_sync()
     do k = 1, NF
        call a(ia(k))%read_from_device()
        call b(ib(k))%read_from_device()
        if (any(transfer(a(ia(k))%data, 1_c_int64_t, size(a(ia(k))%data)) /= &
                transfer(b(ib(k))%data, 1_c_int64_t, size(b(ib(k))%data)))) then
           write(*, '("G: step ",i0," ",a," differs")') step, trim(names(k))
           ndiff = ndiff + 1
        end if
     end do
     if (step == 3) then
        if (all(a(ia(4))%data == -7.0_go_wp)) write(*, '("G: ua never written")')
     end if
     call rotate(ia);  call rotate(ib)
  end do
  write(*, '("G: steps compared, ",i0," arrays differ")') ndiff
  call gocean_finalise()

contains

  ! set A: the single-domain one-call wrapper
  subroutine sequence(open)
    logical, intent(in) :: open
    if (open) then
       call invoke_nemolite_step(prm, a(ia(1)), a(ia(2)), a(ia(3)), a(ia(4)), a(ia(5)), a(ia(6)), a(ia(7)), a(ia(8)), &
                                 a(ia(9)), a(ia(10)), a(ia(11)), a(ia(12)), a(ia(13)), ssh_bc)
    else
       call invoke_nemolite_step(prm, a(ia(1)), a(ia(2)), a(ia(3)), a(ia(4)), a(ia(5)), a(ia(6)), a(ia(7)), a(ia(8)), &
                                 a(ia(9)), a(ia(10)), a(ia(11)), a(ia(12)), a(ia(13)))
    end if
  end subroutine sequence

  ! the new level becomes the old one: un <-> ua, vn <-> va, sshn_t <-> ssha, sshn_u <-> ssha_u, sshn_v <-> ssha_v
  subroutine rotate(ix)
    integer, intent(inout) :: ix(NF)
    integer :: t, p
    integer, parameter :: pa(5) = (/6, 7, 11, 12, 13/), pb(5) = (/4, 5, 1, 2, 3/)
    do p = 1, 5
       t = ix(pa(p));  ix(pa(p)) = ix(pb(p));  ix(pb(p)) = t
    end do
  end subroutine rotate

end program ftest_nemolite_step_dm
