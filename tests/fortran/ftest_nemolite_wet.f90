!> GPU test of the Fortran wrappers of the NEMOLite2D-class time step that skips land (DESIGN.md section 6.9;
!! tests/test_gpu_fortran_nemolite_wet.py).  A channel -- open (-1) first and last internal columns, land rows north and south,
!! an island and a land block 420 columns wide -- with momentum_coriolis; two sets of fields from the same start, rotating by
!! reference: set A through invoke_nemolite_step, set B through invoke_nemolite_step with skip_land = .true.: three tidal
!! steps, one closed-basin step, then one step of invoke_nemolite_step_dm each way.  After every step, per the contract:
!! ssha_u, ssha_v, ua, va and every input hold the same bits in every cell, ssha and sshn_t wherever tmask /= 0.  Prints the
!! plan's counts, the number of land cells whose ssha the two sets hold differently after the first step (the step did skip),
!! and whether the sets agree.
!!   ftest_nemolite_wet.exe NX NY
program ftest_nemolite_wet
  use iso_c_binding
  use kind_params_mod
  use parallel_mod
  use grid_mod
  use field_mod
  use gocean_mod
  use dlesm_hip_mod, only: dlesm_wet_plan_counts
  use dlesm_psy_mod
  implicit none
  integer, parameter :: NF = 13
  ! 1 ssha 2 ssha_u 3 ssha_v 4 ua 5 va 6 un 7 vn 8 ht 9 hu 10 hv 11 sshn_t 12 sshn_u 13 sshn_v
  integer, parameter :: pts(NF) = (/GO_T_POINTS, GO_U_POINTS, GO_V_POINTS, GO_U_POINTS, GO_V_POINTS, GO_U_POINTS, &
                                    GO_V_POINTS, GO_T_POINTS, GO_U_POINTS, GO_V_POINTS, GO_T_POINTS, GO_U_POINTS, GO_V_POINTS/)
  character(len=8), parameter :: names(NF) = (/'ssha    ', 'ssha_u  ', 'ssha_v  ', 'ua      ', 'va      ', 'un      ', &
                                               'vn      ', 'ht      ', 'hu      ', 'hv      ', 'sshn_t  ', 'sshn_u  ', &
                                               'sshn_v  '/)
  character(len=256) :: arg
  integer :: nx, ny, k, step, xs, xe, ys, ye, ndiff, nkept
  integer :: ia(NF), ib(NF)
  integer(c_long_long) :: tiles, active
  integer(c_int) :: rc
  integer, allocatable :: tmask(:,:)
  logical, allocatable :: differ(:,:)
  type(grid_type), target :: g
  type(r2d_field), target :: a(NF), b(NF)
  type(c_momentum_params) :: prm
  real(go_wp) :: ssh_bc
  real(go_wp), parameter :: pi = 3.14159265358979323846_go_wp

  call get_command_argument(1, arg); read(arg, *) nx
  call get_command_argument(2, arg); read(arg, *) ny
  call gocean_initialise()
  g = grid_type(GO_ARAKAWA_C, (/GO_BC_EXTERNAL, GO_BC_EXTERNAL, GO_BC_NONE/), GO_OFFSET_NE)
  call g%decompose(nx, ny)
  xs = g%subdomain%internal%xstart;  xe = g%subdomain%internal%xstop
  ys = g%subdomain%internal%ystart;  ye = g%subdomain%internal%ystop
  allocate(tmask(xe + 1, ye + 1))
  tmask = 1
  tmask(xs - 1, :) = 0;  tmask(xe + 1, :) = 0
  tmask(:, ys - 1) = 0;  tmask(:, ys) = 0;  tmask(:, ye) = 0;  tmask(:, ye + 1) = 0
  tmask(xs, ys + 1:ye - 1) = -1;  tmask(xe, ys + 1:ye - 1) = -1
  tmask(xs + 20:xs + 24, ys + ny / 3:ys + ny / 3 + 3) = 0                 ! an island
  tmask(xs + 60:xs + 479, ys + 4:ye - 6) = 0                               ! a land block 420 columns wide
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
  call momentum_coriolis(g, 7.292116e-5_go_wp, pi / 180.0_go_wp)

  rc = dlesm_wet_plan_counts(wet_plan(g), tiles, active)
  if (rc /= 0) call gocean_stop('ftest_nemolite_wet: dlesm_wet_plan_counts failed')
  write(*, '("G: wet plan: ",i0," tiles, ",i0," active")') tiles, active

  allocate(differ(size(a(1)%data, 1), size(a(1)%data, 2)))
  ndiff = 0
  do step = 1, 5
     if (step <= 3) then
        ssh_bc = tide_ssh(0.1_go_wp, 2.0_go_wp * pi / 43200.0_go_wp, 20.0_go_wp * step)
        call invoke_nemolite_step(prm, a(ia(1)), a(ia(2)), a(ia(3)), a(ia(4)), a(ia(5)), a(ia(6)), a(ia(7)), a(ia(8)), &
                                  a(ia(9)), a(ia(10)), a(ia(11)), a(ia(12)), a(ia(13)), ssh_bc)
        call invoke_nemolite_step(prm, b(ib(1)), b(ib(2)), b(ib(3)), b(ib(4)), b(ib(5)), b(ib(6)), b(ib(7)), b(ib(8)), &
                                  b(ib(9)), b(ib(10)), b(ib(11)), b(ib(12)), b(ib(13)), ssh_bc, skip_land=.true.)
     else if (step == 4) then
        call invoke_nemolite_step(prm, a(ia(1)), a(ia(2)), a(ia(3)), a(ia(4)), a(ia(5)), a(ia(6)), a(ia(7)), a(ia(8)), &
                                  a(ia(9)), a(ia(10)), a(ia(11)), a(ia(12)), a(ia(13)), skip_land=.false.)
        call invoke_nemolite_step(prm, b(ib(1)), b(ib(2)), b(ib(3)), b(ib(4)), b(ib(5)), b(ib(6)), b(ib(7)), b(ib(8)), &
                                  b(ib(9)), b(ib(10)), b(ib(11)), b(ib(12)), b(ib(13)), skip_land=.true.)
     else
        ssh_bc = tide_ssh(0.1_go_wp, 2.0_go_wp * pi / 43200.0_go_wp, 20.0_go_wp * step)
        call invoke_nemolite_step_dm(prm, a(ia(1)), a(ia(2)), a(ia(3)), a(ia(4)), a(ia(5)), a(ia(6)), a(ia(7)), a(ia(8)), &
                                     a(ia(9)), a(ia(10)), a(ia(11)), a(ia(12)), a(ia(13)), ssh_bc)
        call invoke_nemolite_step_dm(prm, b(ib(1)), b(ib(2)), b(ib(3)), b(ib(4)), b(ib(5)), b(ib(6)), b(ib(7)), b(ib(8)), &
                                     b(ib(9)), b(ib(10)), b(ib(11)), b(ib(12)), b(ib(13)), ssh_bc, skip_land=.true.)
     end if
     call device_sync()
     do k = 1, NF
        call a(ia(k))%read_from_device()
        call b(ib(k))%read_from_device()
        differ = reshape(transfer(a(ia(k))%data, 1_c_int64_t, size(differ)) /= &
                         transfer(b(ib(k))%data, 1_c_int64_t, size(differ)), shape(differ))
        if (k == 1 .and. step == 1) then
           nkept = count(differ .and. g%tmask == 0)
           write(*, '("G: land ssha kept in ",i0," cells")') nkept
        end if
        if (k == 1 .or. k == 11) differ = differ .and. g%tmask /= 0     ! ssha, and sshn_t it rotates into: land may be stale
        if (any(differ)) then
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

  ! the new level becomes the old one: un <-> ua, vn <-> va, sshn_t <-> ssha, sshn_u <-> ssha_u, sshn_v <-> ssha_v
  subroutine rotate(ix)
    integer, intent(inout) :: ix(NF)
    integer :: t, p
    integer, parameter :: pa(5) = (/6, 7, 11, 12, 13/), pb(5) = (/4, 5, 1, 2, 3/)
    do p = 1, 5
       t = ix(pa(p));  ix(pa(p)) = ix(pb(p));  ix(pb(p)) = t
    end do
  end subroutine rotate

end program ftest_nemolite_wet
