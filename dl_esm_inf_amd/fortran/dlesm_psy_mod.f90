!> PSy-layer building blocks for HIP: what replaces the generated
!!     do jj = fld%internal%ystart, fld%internal%ystop
!!        do ji = fld%internal%xstart, fld%internal%xstop
!!           call kern_code(ji, jj, out%data, in%data, ...)
!! loop nests (form: reference infrastructure_mod.f90:32-41) -- one call that launches the
!! matching CDNA4 kernel over the same index box on the fields' device copies.
!!
!! Also provides infrastructure_mod, the reference's field-copy "kernel" module, with its
!! metadata type and pointwise code unchanged in meaning.
module infrastructure_mod
  use kind_params_mod
  use kernel_mod
  use argument_mod
  use grid_mod
  use field_mod
  implicit none

  type, extends(kernel_type) :: copy
     type(go_arg), dimension(2) :: meta_args = &
          (/ go_arg(GO_WRITE, GO_EVERY, GO_POINTWISE), &
             go_arg(GO_READ,  GO_EVERY, GO_POINTWISE) /)
     integer :: ITERATES_OVER = GO_ALL_PTS
     integer :: index_offset = GO_OFFSET_ANY
   contains
     procedure, nopass :: code => field_copy_code
  end type copy

contains

  subroutine field_copy_code(ji, jj, output, input)
    integer, intent(in) :: ji, jj
    real(go_wp), dimension(:,:), intent(in) :: input
    real(go_wp), dimension(:,:), intent(out) :: output
    output(ji, jj) = input(ji, jj)
  end subroutine field_copy_code

end module infrastructure_mod


module dlesm_psy_mod
  use iso_c_binding
  use kind_params_mod
  use grid_mod
  use field_mod
  use gocean_mod, only: gocean_stop
  use dlesm_hip_mod
  implicit none
  private

  public :: invoke_jacobi5_masked, invoke_jacobi5_dm_pipelined, halo_join, halo_connect_peers, invoke_jacobi5_residual
  public :: invoke_shallow_step_sw, invoke_periodic_halos, invoke_stencil9, invoke_stencil9_dm
  public :: invoke_jacobi5, invoke_jacobi5_dm, invoke_shallow_step, invoke_copy, invoke_hash_init
  public :: invoke_shallow_step_dm_pipelined, invoke_continuity
  public :: momentum_params, c_momentum_params, momentum_coriolis, invoke_momentum_u, invoke_momentum_v, invoke_momentum
  public :: invoke_next_sshu, invoke_next_sshv
  public :: open_boundary, tide_ssh, invoke_bc_ssh, invoke_bc_flather_u, invoke_bc_flather_v, invoke_bc_open
  public :: invoke_nemolite_step, invoke_nemolite_step_dm, wet_plan
  public :: invoke_tracer_step, invoke_tracer_step_dm, invoke_tracer_step_muscl, invoke_tracer_step_muscl_dm
  public :: invoke_tracer_step_hancock, invoke_tracer_step_hancock_dm
  public :: invoke_nemolite_coupled_step_dm
  public :: tracer_courant, tracer_courant_type
  public :: flow_courant, flow_courant_type
  public :: flow_output
  public :: drifters_type, drifters_create, drifters_get, drifters_free, drifter_step
  public :: particle_sort, particle_origin
  public :: dispersal_step, random_walk
  public :: cell_bin
  public :: DLESM_DRIFTER_ACTIVE, DLESM_DRIFTER_LEFT, DLESM_DRIFTER_OPEN, DLESM_DRIFTER_GROUNDED, DLESM_DRIFTER_FREE
  public :: invoke_shallow_step_dm, halo_exchange_multi, invoke_jacobi5_multi, plan_jacobi5, plan_shallow_step
  public :: shallow_params, c_sw_params, device_sync, grid_to_device
  public :: invoke_compute_cu, invoke_compute_cv, invoke_compute_z, invoke_compute_h
  public :: invoke_compute_unew, invoke_compute_vnew, invoke_compute_pnew, invoke_time_smooth
  public :: invoke_shallow_step_sw_periodic, plan_shallow_step_sw, invoke_periodic_halos_multi
  public :: invoke_shallow_step_smooth, invoke_shallow_step_sw_smooth_periodic, invoke_shallow_step_smooth_dm
  public :: invoke_shallow_step_x2, invoke_shallow_step_smooth_x2
  public :: invoke_shallow_step_x2_dm, invoke_shallow_step_smooth_x2_dm
  public :: invoke_shallow_step_sw_x2_periodic, invoke_shallow_step_sw_smooth_x2_periodic

contains

  subroutine device_sync()
    if (hipDeviceSynchronize() /= 0) call gocean_stop('device synchronisation failed')
  end subroutine device_sync

  subroutine need_device(f)
    type(r2d_field), intent(inout), target :: f
    if (.not. f%data_on_device) call field_to_device(f)
    if (.not. field_on_dlesm_device(f)) call gocean_stop('PSy layer: field lives on a foreign device')
  end subroutine need_device

  !> out = 0.25*((w+e)+(s+n)) of `in` over out%internal
  subroutine invoke_jacobi5(out, in)
    type(r2d_field), intent(inout), target :: out, in
    integer(c_int) :: rc
    call need_device(in);  call need_device(out)
    rc = dlesm_stencil5_f64(field_device_data(in), field_device_data(out), &
                            int(out%grid%nx, c_int), int(out%grid%ny, c_int), &
                            int(out%internal%xstart, c_int), int(out%internal%xstop, c_int), &
                            int(out%internal%ystart, c_int), int(out%internal%ystop, c_int), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_jacobi5: ' // dlesm_error_text())
  end subroutine invoke_jacobi5

  !> A general 3x3 weighted stencil: out(ji,jj) = SUM coef(di,dj)*in(ji+di,jj+dj) over out%internal --
  !! the PSy layer of a kernel with a GO_STENCIL(111,111,111) read argument and nine real scalars.
  subroutine invoke_stencil9(out, in, coef)
    type(r2d_field), intent(inout), target :: out, in
    real(go_wp), intent(in) :: coef(-1:1, -1:1)
    real(c_double) :: c9(9)
    integer(c_int) :: rc
    integer :: di, dj
    call need_device(in);  call need_device(out)
    ! di fastest, south row first: the C order coef[(dj+1)*3 + (di+1)].  (Explicit loops: amdflang 22 -O2
    ! turns reshape() of an array with lower bounds -1 into a broadcast of its first element.)
    do dj = -1, 1
       do di = -1, 1
          c9(3 * (dj + 1) + di + 2) = coef(di, dj)
       end do
    end do
    rc = dlesm_stencil9_f64(field_device_data(in), field_device_data(out), c9, &
                            int(out%grid%nx, c_int), int(out%grid%ny, c_int), &
                            int(out%internal%xstart, c_int), int(out%internal%xstop, c_int), &
                            int(out%internal%ystart, c_int), int(out%internal%ystop, c_int), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_stencil9: ' // dlesm_error_text())
  end subroutine invoke_stencil9

  !> invoke_stencil9 + out%halo_exchange(1), the exchange hidden behind the interior sweep
  !! (all eight directions when a corner weight is non-zero, the four edges otherwise).
  subroutine invoke_stencil9_dm(out, in, coef)
    use parallel_comms_mod, only: halo_plan_for
    use parallel_utils_mod, only: DIST_MEM_ENABLED
    type(r2d_field), intent(inout), target :: out, in
    real(go_wp), intent(in) :: coef(-1:1, -1:1)
    real(c_double) :: c9(9)
    integer(c_int) :: rc
    integer :: di, dj
    if (.not. DIST_MEM_ENABLED) then
       call invoke_stencil9(out, in, coef)
       return
    end if
    call need_device(in);  call need_device(out)
    do dj = -1, 1
       do di = -1, 1
          c9(3 * (dj + 1) + di + 2) = coef(di, dj)
       end do
    end do
    rc = dlesm_stencil9_step_dm(halo_plan_for(out%grid%nx, out%grid%ny), field_device_data(in), &
                                field_device_data(out), c9, int(out%grid%nx, c_int), int(out%grid%ny, c_int), &
                                int(out%internal%xstart, c_int), int(out%internal%xstop, c_int), &
                                int(out%internal%ystart, c_int), int(out%internal%ystop, c_int), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_stencil9_dm: ' // dlesm_error_text())
  end subroutine invoke_stencil9_dm

  !> The PSy layer of a kernel whose metadata requests the T mask,
  !!   go_arg(GO_WRITE, GO_CT, GO_POINTWISE), go_arg(GO_READ, GO_CT, GO_STENCIL(010,111,010)),
  !!   go_arg(GO_READ, GO_GRID_MASK_T)                          (argument_mod.f90:75-112)
  !! i.e. `call jacobi5_masked_code(ji, jj, out%data, in%data, out%grid%tmask)` over out%internal:
  !! the kernel gets the grid's mask -- on the device its mirror grid%tmask_device, created on
  !! first use.  Dry points carry their value over, dry neighbours are mirrored.
  subroutine invoke_jacobi5_masked(out, in)
    type(r2d_field), intent(inout), target :: out, in
    integer(c_int) :: rc
    call need_device(in);  call need_device(out)
    if (.not. c_associated(out%grid%tmask_device)) call grid_to_device(out%grid)
    rc = dlesm_stencil5_masked_f64(field_device_data(in), field_device_data(out), out%grid%tmask_device, &
                                   int(out%grid%nx, c_int), int(out%grid%ny, c_int), &
                                   int(out%internal%xstart, c_int), int(out%internal%xstop, c_int), &
                                   int(out%internal%ystart, c_int), int(out%internal%ystop, c_int), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_jacobi5_masked: ' // dlesm_error_text())
  end subroutine invoke_jacobi5_masked

  !> The PSy layer of a kernel on all three point types whose metadata requests the cell area,
  !!   go_arg(GO_WRITE, GO_CT, GO_POINTWISE), go_arg(GO_READ, GO_CT, GO_POINTWISE),
  !!   go_arg(GO_READ, GO_CU, GO_STENCIL(000,110,000)) x 3, go_arg(GO_READ, GO_CV, GO_STENCIL(000,010,010)) x 3,
  !!   go_arg(GO_READ, GO_R_SCALAR, GO_POINTWISE), go_arg(GO_READ, GO_GRID_AREA_T)
  !! i.e. `call continuity_code(ji, jj, ssha%data, sshn_t%data, sshn_u%data, sshn_v%data, hu%data, hv%data,
  !! un%data, vn%data, rdt, ssha%grid%area_t)` over ssha%internal (the free-surface update of a
  !! NEMOLite2D-class model): the kernel gets the grid's area_t, on the device its mirror.
  subroutine invoke_continuity(ssha, sshn_t, sshn_u, sshn_v, hu, hv, un, vn, rdt)
    type(r2d_field), intent(inout), target :: ssha, sshn_t, sshn_u, sshn_v, hu, hv, un, vn
    real(go_wp), intent(in) :: rdt
    integer(c_int) :: rc
    call need_device(ssha);  call need_device(sshn_t);  call need_device(sshn_u);  call need_device(sshn_v)
    call need_device(hu);  call need_device(hv);  call need_device(un);  call need_device(vn)
    if (.not. c_associated(ssha%grid%area_t_device)) call grid_to_device(ssha%grid)
    rc = dlesm_continuity_f64(real(rdt, c_double), int(ssha%grid%nx, c_int), int(ssha%grid%ny, c_int), &
                              int(ssha%internal%xstart, c_int), int(ssha%internal%xstop, c_int), &
                              int(ssha%internal%ystart, c_int), int(ssha%internal%ystop, c_int), &
                              field_device_data(sshn_t), field_device_data(sshn_u), field_device_data(sshn_v), &
                              field_device_data(hu), field_device_data(hv), field_device_data(un), &
                              field_device_data(vn), ssha%grid%area_t_device, field_device_data(ssha), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_continuity: ' // dlesm_error_text())
  end subroutine invoke_continuity

  !> Constants of the NEMOLite2D-class momentum kernels (DESIGN.md section 6.5): time step, bottom friction
  !! coefficient, viscosity, gravity.
  function momentum_params(rdt, cbfr, visc, g) result(p)
    real(go_wp), intent(in) :: rdt, cbfr, visc, g
    type(c_momentum_params) :: p
    p = c_momentum_params(real(rdt, c_double), real(cbfr, c_double), real(visc, c_double), real(g, c_double))
  end function momentum_params

  !> The Coriolis parameter of the momentum kernels, once per grid (DESIGN.md section 6.5):
  !! fcor_u = (2*omega)*sin(gphiu*d2r) and fcor_v from gphiv, computed on the host and uploaded.  The
  !! kernels never evaluate a transcendental.  Called again, it recomputes and uploads again.
  subroutine momentum_coriolis(grid, omega, d2r)
    type(grid_type), intent(inout), target :: grid
    real(go_wp), intent(in) :: omega, d2r
    integer(c_size_t) :: nb
    if (.not. allocated(grid%gphiu) .or. .not. allocated(grid%gphiv)) &
         call gocean_stop('momentum_coriolis: grid_init has not been called for this grid')
    if (.not. allocated(grid%fcor_u)) allocate(grid%fcor_u(grid%nx, grid%ny), grid%fcor_v(grid%nx, grid%ny))
    grid%fcor_u = (2.0_go_wp * omega) * sin(grid%gphiu * d2r)
    grid%fcor_v = (2.0_go_wp * omega) * sin(grid%gphiv * d2r)
    nb = int(grid%nx, c_size_t) * int(grid%ny, c_size_t) * 8_c_size_t
    if (.not. c_associated(grid%fcor_u_device)) then
       if (hipMalloc(grid%fcor_u_device, nb) /= 0) call gocean_stop('momentum_coriolis: hipMalloc failed')
    end if
    if (.not. c_associated(grid%fcor_v_device)) then
       if (hipMalloc(grid%fcor_v_device, nb) /= 0) call gocean_stop('momentum_coriolis: hipMalloc failed')
    end if
    if (hipMemcpy(grid%fcor_u_device, c_loc(grid%fcor_u), nb, 1_c_int) /= 0 .or. &
        hipMemcpy(grid%fcor_v_device, c_loc(grid%fcor_v), nb, 1_c_int) /= 0) &
         call gocean_stop('momentum_coriolis: upload failed')
  end subroutine momentum_coriolis

  !> the grid's device mirrors as a dlesm_momentum_grid; stops when momentum_coriolis was never called for the grid
  function momentum_grid(grid, who) result(mg)
    type(grid_type), intent(inout), target :: grid
    character(len=*), intent(in) :: who
    type(c_momentum_grid) :: mg
    if (.not. c_associated(grid%fcor_u_device) .or. .not. c_associated(grid%fcor_v_device)) &
         call gocean_stop(who // ': the Coriolis parameter of this grid has not been set: call momentum_coriolis first')
    call grid_to_device(grid)
    mg = c_momentum_grid(grid%tmask_device, grid%dx_t_device, grid%dy_t_device, grid%dx_u_device, grid%dy_u_device, &
                         grid%dx_v_device, grid%dy_v_device, grid%area_u_device, grid%area_v_device, &
                         grid%fcor_u_device, grid%fcor_v_device)
  end function momentum_grid

  !> momentum_u (DESIGN.md section 6.5) over ua%internal: ua where both T cells of the u face are wet.  The
  !! kernel gets the grid's metric mirrors and the Coriolis parameter momentum_coriolis set.
  subroutine invoke_momentum_u(params, ua, un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u)
    type(c_momentum_params), intent(in) :: params
    type(r2d_field), intent(inout), target :: ua, un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u
    type(c_momentum_grid) :: mg
    integer(c_int) :: rc
    call need_device(ua);  call need_device(un);  call need_device(vn);  call need_device(ht);  call need_device(sshn_t)
    call need_device(hu);  call need_device(sshn_u);  call need_device(hv);  call need_device(sshn_v)
    call need_device(ssha_u)
    mg = momentum_grid(ua%grid, 'invoke_momentum_u')
    rc = dlesm_momentum_u_f64(params, mg, int(ua%grid%nx, c_int), int(ua%grid%ny, c_int), &
                              int(ua%internal%xstart, c_int), int(ua%internal%xstop, c_int), &
                              int(ua%internal%ystart, c_int), int(ua%internal%ystop, c_int), &
                              field_device_data(un), field_device_data(vn), field_device_data(ht), field_device_data(sshn_t), &
                              field_device_data(hu), field_device_data(sshn_u), field_device_data(hv), &
                              field_device_data(sshn_v), field_device_data(ssha_u), field_device_data(ua), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_momentum_u: ' // dlesm_error_text())
  end subroutine invoke_momentum_u

  !> momentum_v (DESIGN.md section 6.5) over va%internal: va where both T cells of the v face are wet
  subroutine invoke_momentum_v(params, va, un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_v)
    type(c_momentum_params), intent(in) :: params
    type(r2d_field), intent(inout), target :: va, un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_v
    type(c_momentum_grid) :: mg
    integer(c_int) :: rc
    call need_device(va);  call need_device(un);  call need_device(vn);  call need_device(ht);  call need_device(sshn_t)
    call need_device(hu);  call need_device(sshn_u);  call need_device(hv);  call need_device(sshn_v)
    call need_device(ssha_v)
    mg = momentum_grid(va%grid, 'invoke_momentum_v')
    rc = dlesm_momentum_v_f64(params, mg, int(va%grid%nx, c_int), int(va%grid%ny, c_int), &
                              int(va%internal%xstart, c_int), int(va%internal%xstop, c_int), &
                              int(va%internal%ystart, c_int), int(va%internal%ystop, c_int), &
                              field_device_data(un), field_device_data(vn), field_device_data(ht), field_device_data(sshn_t), &
                              field_device_data(hu), field_device_data(sshn_u), field_device_data(hv), &
                              field_device_data(sshn_v), field_device_data(ssha_v), field_device_data(va), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_momentum_v: ' // dlesm_error_text())
  end subroutine invoke_momentum_v

  !> Both momentum loop nests in one sweep: momentum_u over ua%internal and momentum_v over va%internal, bit for
  !! bit invoke_momentum_u followed by invoke_momentum_v, at 180 instead of 2 x 140 B/cell.
  subroutine invoke_momentum(params, ua, va, un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, ssha_v)
    type(c_momentum_params), intent(in) :: params
    type(r2d_field), intent(inout), target :: ua, va, un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, ssha_v
    type(c_momentum_grid) :: mg
    type(c_region) :: ubox, vbox
    integer(c_int) :: rc
    call need_device(ua);  call need_device(va);  call need_device(un);  call need_device(vn);  call need_device(ht)
    call need_device(sshn_t);  call need_device(hu);  call need_device(sshn_u);  call need_device(hv)
    call need_device(sshn_v);  call need_device(ssha_u);  call need_device(ssha_v)
    mg = momentum_grid(ua%grid, 'invoke_momentum')
    ubox = c_region(ua%internal%nx, ua%internal%ny, ua%internal%xstart, ua%internal%xstop, &
                    ua%internal%ystart, ua%internal%ystop)
    vbox = c_region(va%internal%nx, va%internal%ny, va%internal%xstart, va%internal%xstop, &
                    va%internal%ystart, va%internal%ystop)
    rc = dlesm_momentum_f64(params, mg, int(ua%grid%nx, c_int), int(ua%grid%ny, c_int), ubox, vbox, &
                            field_device_data(un), field_device_data(vn), field_device_data(ht), field_device_data(sshn_t), &
                            field_device_data(hu), field_device_data(sshn_u), field_device_data(hv), &
                            field_device_data(sshn_v), field_device_data(ssha_u), field_device_data(ssha_v), &
                            field_device_data(ua), field_device_data(va), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_momentum: ' // dlesm_error_text())
  end subroutine invoke_momentum

  !> next_sshu (DESIGN.md section 6.5) over sshn_u%internal, from sshn_t and the grid's tmask, area_t and area_u
  subroutine invoke_next_sshu(sshn_u, sshn_t)
    type(r2d_field), intent(inout), target :: sshn_u, sshn_t
    integer(c_int) :: rc
    call need_device(sshn_u);  call need_device(sshn_t)
    call grid_to_device(sshn_u%grid)
    rc = dlesm_next_sshu_f64(int(sshn_u%grid%nx, c_int), int(sshn_u%grid%ny, c_int), &
                             int(sshn_u%internal%xstart, c_int), int(sshn_u%internal%xstop, c_int), &
                             int(sshn_u%internal%ystart, c_int), int(sshn_u%internal%ystop, c_int), &
                             sshn_u%grid%tmask_device, sshn_u%grid%area_t_device, sshn_u%grid%area_u_device, &
                             field_device_data(sshn_t), field_device_data(sshn_u), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_next_sshu: ' // dlesm_error_text())
  end subroutine invoke_next_sshu

  !> next_sshv (DESIGN.md section 6.5) over sshn_v%internal, from sshn_t and the grid's tmask, area_t and area_v
  subroutine invoke_next_sshv(sshn_v, sshn_t)
    type(r2d_field), intent(inout), target :: sshn_v, sshn_t
    integer(c_int) :: rc
    call need_device(sshn_v);  call need_device(sshn_t)
    call grid_to_device(sshn_v%grid)
    rc = dlesm_next_sshv_f64(int(sshn_v%grid%nx, c_int), int(sshn_v%grid%ny, c_int), &
                             int(sshn_v%internal%xstart, c_int), int(sshn_v%internal%xstop, c_int), &
                             int(sshn_v%internal%ystart, c_int), int(sshn_v%internal%ystop, c_int), &
                             sshn_v%grid%tmask_device, sshn_v%grid%area_t_device, sshn_v%grid%area_v_device, &
                             field_device_data(sshn_t), field_device_data(sshn_v), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_next_sshv: ' // dlesm_error_text())
  end subroutine invoke_next_sshv

  !> The open-boundary plan of a grid (DESIGN.md section 6.6), made once from the host tmask and the T-, U- and V-point
  !! internal regions: the lists of open T cells, open u faces and open v faces.  Stops if the library refuses the mask (an
  !! open face whose inner face is open -- a wet region one cell wide between two open cells -- or lies at the edge of the
  !! array).
  function open_boundary(grid) result(plan)
    type(grid_type), intent(inout), target :: grid
    type(c_ptr) :: plan
    type(c_region) :: sub, box(3), whole
    integer, parameter :: pts(3) = (/GO_T_POINTS, GO_U_POINTS, GO_V_POINTS/)
    integer :: k
    integer(c_int) :: rc
    if (.not. c_associated(grid%obc)) then
       if (.not. allocated(grid%tmask)) call gocean_stop('open_boundary: grid_init has not been called for this grid')
       associate (s => grid%subdomain%internal)
         sub = c_region(s%nx, s%ny, s%xstart, s%xstop, s%ystart, s%ystop)
       end associate
       do k = 1, 3                    ! the internal regions of T, U and V fields (set_field_bounds)
          rc = dlesm_field_bounds(int(pts(k), c_int), int(grid%offset, c_int), int(grid%boundary_conditions(1), c_int), &
                                  int(grid%boundary_conditions(2), c_int), sub, int(grid%nx, c_int), int(grid%ny, c_int), &
                                  box(k), whole)
          if (rc /= 0) call gocean_stop('open_boundary: ' // dlesm_error_text())
       end do
       rc = dlesm_obc_create(c_loc(grid%tmask), int(grid%nx, c_int), int(grid%ny, c_int), box(1), box(2), box(3), grid%obc)
       if (rc /= 0) call gocean_stop('open_boundary: ' // dlesm_error_text())
    end if
    plan = grid%obc
  end function open_boundary

  !> The wet plan of a grid (DESIGN.md section 6.9), made once from the host tmask -- the mask grid_to_device mirrors -- and the
  !! T-point internal region: which wave tiles of the one-sweep step store anything but land ssha.
  function wet_plan(grid) result(plan)
    type(grid_type), intent(inout), target :: grid
    type(c_ptr) :: plan
    type(c_region) :: sub, box, whole
    integer(c_int) :: rc
    if (.not. c_associated(grid%wet)) then
       if (.not. allocated(grid%tmask)) call gocean_stop('wet_plan: grid_init has not been called for this grid')
       associate (s => grid%subdomain%internal)
         sub = c_region(s%nx, s%ny, s%xstart, s%xstop, s%ystart, s%ystop)
       end associate
       rc = dlesm_field_bounds(int(GO_T_POINTS, c_int), int(grid%offset, c_int), int(grid%boundary_conditions(1), c_int), &
                               int(grid%boundary_conditions(2), c_int), sub, int(grid%nx, c_int), int(grid%ny, c_int), &
                               box, whole)
       if (rc /= 0) call gocean_stop('wet_plan: ' // dlesm_error_text())
       rc = dlesm_wet_plan_create(c_loc(grid%tmask), int(grid%nx, c_int), int(grid%ny, c_int), box, grid%wet)
       if (rc /= 0) call gocean_stop('wet_plan: ' // dlesm_error_text())
    end if
    plan = grid%wet
  end function wet_plan

  !> The boundary sea-surface height of bc_ssh, amp*sin(omega*t), with the host's sin (DESIGN.md section 6.6)
  function tide_ssh(amp, omega, t) result(ssh_bc)
    real(go_wp), intent(in) :: amp, omega, t
    real(go_wp) :: ssh_bc
    ssh_bc = amp * sin(omega * t)
  end function tide_ssh

  !> bc_ssh (DESIGN.md section 6.6): ssha = ssh_bc on the open T cells of ssha%internal
  subroutine invoke_bc_ssh(ssha, ssh_bc)
    type(r2d_field), intent(inout), target :: ssha
    real(go_wp), intent(in) :: ssh_bc
    integer(c_int) :: rc
    call need_device(ssha)
    rc = dlesm_bc_ssh_f64(open_boundary(ssha%grid), real(ssh_bc, c_double), field_device_data(ssha), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_bc_ssh: ' // dlesm_error_text())
  end subroutine invoke_bc_ssh

  !> Flather on the open u faces of ua%internal (DESIGN.md section 6.6), ua in place
  subroutine invoke_bc_flather_u(params, ua, hu, sshn_u, sshn_t)
    type(c_momentum_params), intent(in) :: params
    type(r2d_field), intent(inout), target :: ua, hu, sshn_u, sshn_t
    integer(c_int) :: rc
    call need_device(ua);  call need_device(hu);  call need_device(sshn_u);  call need_device(sshn_t)
    rc = dlesm_bc_flather_u_f64(open_boundary(ua%grid), params, field_device_data(hu), field_device_data(sshn_u), &
                                field_device_data(sshn_t), field_device_data(ua), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_bc_flather_u: ' // dlesm_error_text())
  end subroutine invoke_bc_flather_u

  !> Flather on the open v faces of va%internal (DESIGN.md section 6.6), va in place
  subroutine invoke_bc_flather_v(params, va, hv, sshn_v, sshn_t)
    type(c_momentum_params), intent(in) :: params
    type(r2d_field), intent(inout), target :: va, hv, sshn_v, sshn_t
    integer(c_int) :: rc
    call need_device(va);  call need_device(hv);  call need_device(sshn_v);  call need_device(sshn_t)
    rc = dlesm_bc_flather_v_f64(open_boundary(va%grid), params, field_device_data(hv), field_device_data(sshn_v), &
                                field_device_data(sshn_t), field_device_data(va), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_bc_flather_v: ' // dlesm_error_text())
  end subroutine invoke_bc_flather_v

  !> bc_ssh, Flather on u and Flather on v in one launch, bit for bit the three separate wrappers (DESIGN.md section 6.6)
  subroutine invoke_bc_open(params, ssh_bc, ssha, ua, va, hu, sshn_u, hv, sshn_v, sshn_t)
    type(c_momentum_params), intent(in) :: params
    real(go_wp), intent(in) :: ssh_bc
    type(r2d_field), intent(inout), target :: ssha, ua, va, hu, sshn_u, hv, sshn_v, sshn_t
    integer(c_int) :: rc
    call need_device(ssha);  call need_device(ua);  call need_device(va);  call need_device(hu);  call need_device(sshn_u)
    call need_device(hv);  call need_device(sshn_v);  call need_device(sshn_t)
    rc = dlesm_bc_open_f64(open_boundary(ssha%grid), params, real(ssh_bc, c_double), field_device_data(hu), &
                           field_device_data(sshn_u), field_device_data(hv), field_device_data(sshn_v), &
                           field_device_data(sshn_t), field_device_data(ssha), field_device_data(ua), &
                           field_device_data(va), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_bc_open: ' // dlesm_error_text())
  end subroutine invoke_bc_open

  !> One NEMOLite2D-class time step in one call (DESIGN.md section 6.7): bit for bit invoke_continuity (rdt = params%rdt),
  !! invoke_next_sshu and invoke_next_sshv on ssha, invoke_momentum and, when ssh_bc is present, invoke_bc_open on the grid's
  !! open_boundary plan (absent: a closed basin, no boundary pass).  ssha is in/out: the faces at the east and north edge of
  !! the box read ssha in the ring.  Stops without momentum_coriolis, and on a decomposed grid (the sequence needs an ssha
  !! halo exchange between continuity and next_ssh*: use the separate wrappers there).
  !! skip_land present and true: the sweep leaves out the wave tiles of the grid's wet_plan that hold nothing but land (DESIGN.md
  !! section 6.9): ssha_u, ssha_v, ua and va as without it in every cell, ssha in every cell with tmask /= 0; a land cell of
  !! ssha may keep its content.
  subroutine invoke_nemolite_step(params, ssha, ssha_u, ssha_v, ua, va, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, ssh_bc, &
                                  skip_land)
    type(c_momentum_params), intent(in) :: params
    type(r2d_field), intent(inout), target :: ssha, ssha_u, ssha_v, ua, va, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v
    real(go_wp), intent(in), optional :: ssh_bc
    logical, intent(in), optional :: skip_land
    type(c_momentum_grid) :: mg
    type(c_region) :: tbox, ubox, vbox
    type(c_ptr) :: plan, wet
    real(c_double) :: bc
    integer(c_int) :: rc
    if (ssha%grid%decomp%ndomains > 1) &
         call gocean_stop('invoke_nemolite_step: the grid is decomposed: the step needs an ssha halo exchange between ' // &
                          'continuity and next_ssh*, which one call cannot hold; use the separate wrappers')
    call need_device(ssha);  call need_device(ssha_u);  call need_device(ssha_v);  call need_device(ua);  call need_device(va)
    call need_device(un);  call need_device(vn);  call need_device(ht);  call need_device(hu);  call need_device(hv)
    call need_device(sshn_t);  call need_device(sshn_u);  call need_device(sshn_v)
    mg = momentum_grid(ssha%grid, 'invoke_nemolite_step')
    tbox = c_region(ssha%internal%nx, ssha%internal%ny, ssha%internal%xstart, ssha%internal%xstop, &
                    ssha%internal%ystart, ssha%internal%ystop)
    ubox = c_region(ua%internal%nx, ua%internal%ny, ua%internal%xstart, ua%internal%xstop, &
                    ua%internal%ystart, ua%internal%ystop)
    vbox = c_region(va%internal%nx, va%internal%ny, va%internal%xstart, va%internal%xstop, &
                    va%internal%ystart, va%internal%ystop)
    plan = c_null_ptr
    bc = 0.0_c_double
    if (present(ssh_bc)) then
       plan = open_boundary(ssha%grid)
       bc = real(ssh_bc, c_double)
    end if
    wet = c_null_ptr
    if (present(skip_land)) then
       if (skip_land) wet = wet_plan(ssha%grid)
    end if
    if (c_associated(wet)) then
       rc = dlesm_nemolite_step_wet_f64(wet, params, mg, ssha%grid%area_t_device, int(ssha%grid%nx, c_int), &
                                        int(ssha%grid%ny, c_int), tbox, ubox, vbox, plan, bc, field_device_data(un), &
                                        field_device_data(vn), field_device_data(ht), field_device_data(hu), &
                                        field_device_data(hv), field_device_data(sshn_t), field_device_data(sshn_u), &
                                        field_device_data(sshn_v), field_device_data(ssha), field_device_data(ssha_u), &
                                        field_device_data(ssha_v), field_device_data(ua), field_device_data(va), c_null_ptr)
    else
       rc = dlesm_nemolite_step_f64(params, mg, ssha%grid%area_t_device, int(ssha%grid%nx, c_int), int(ssha%grid%ny, c_int), &
                                    tbox, ubox, vbox, plan, bc, field_device_data(un), field_device_data(vn), &
                                    field_device_data(ht), field_device_data(hu), field_device_data(hv), &
                                    field_device_data(sshn_t), field_device_data(sshn_u), field_device_data(sshn_v), &
                                    field_device_data(ssha), field_device_data(ssha_u), field_device_data(ssha_v), &
                                    field_device_data(ua), field_device_data(va), c_null_ptr)
    end if
    if (rc /= 0) call gocean_stop('invoke_nemolite_step: ' // dlesm_error_text())
  end subroutine invoke_nemolite_step

  !> One NEMOLite2D-class time step and ONE exchange of its five outputs on a decomposed grid (dlesm_nemolite_step_dm, DESIGN.md
  !! section 6.8): bit for bit invoke_continuity, ssha%halo_exchange(1), invoke_next_sshu / invoke_next_sshv, invoke_momentum,
  !! (ssh_bc present) invoke_bc_open on this rank's open_boundary plan, then the exchange of ssha, ssha_u, ssha_v, ua, va.  The
  !! inputs need valid depth-1 halos, corners included; the outputs leave with them.  Collective.  The grid must have been
  !! decomposed with halo_width = 1 (without distributed memory the plan has no messages: invoke_nemolite_step, bit for bit).
  !! Stops on another halo width and without momentum_coriolis.
  !! skip_land present and true: as invoke_nemolite_step, with this rank's wet_plan (dlesm_nemolite_step_wet_dm, section 6.9).
  subroutine invoke_nemolite_step_dm(params, ssha, ssha_u, ssha_v, ua, va, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, ssh_bc, &
                                     skip_land)
    use parallel_comms_mod, only: halo_plan_for, serial_plan_for
    use parallel_utils_mod, only: DIST_MEM_ENABLED
    type(c_momentum_params), intent(in) :: params
    type(r2d_field), intent(inout), target :: ssha, ssha_u, ssha_v, ua, va, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v
    real(go_wp), intent(in), optional :: ssh_bc
    logical, intent(in), optional :: skip_land
    type(c_momentum_grid) :: mg
    type(c_region) :: tbox, ubox, vbox
    type(c_ptr) :: plan, obc, wet
    real(c_double) :: bc
    integer(c_int) :: rc
    if (ssha%grid%subdomain%internal%xstart - 1 /= 1 .or. ssha%grid%subdomain%internal%ystart - 1 /= 1) &
         call gocean_stop('invoke_nemolite_step_dm: the grid must be decomposed with halo_width = 1')
    call need_device(ssha);  call need_device(ssha_u);  call need_device(ssha_v);  call need_device(ua);  call need_device(va)
    call need_device(un);  call need_device(vn);  call need_device(ht);  call need_device(hu);  call need_device(hv)
    call need_device(sshn_t);  call need_device(sshn_u);  call need_device(sshn_v)
    mg = momentum_grid(ssha%grid, 'invoke_nemolite_step_dm')
    tbox = c_region(ssha%internal%nx, ssha%internal%ny, ssha%internal%xstart, ssha%internal%xstop, &
                    ssha%internal%ystart, ssha%internal%ystop)
    ubox = c_region(ua%internal%nx, ua%internal%ny, ua%internal%xstart, ua%internal%xstop, &
                    ua%internal%ystart, ua%internal%ystop)
    vbox = c_region(va%internal%nx, va%internal%ny, va%internal%xstart, va%internal%xstop, &
                    va%internal%ystart, va%internal%ystop)
    obc = c_null_ptr
    bc = 0.0_c_double
    if (present(ssh_bc)) then
       obc = open_boundary(ssha%grid)
       bc = real(ssh_bc, c_double)
    end if
    if (DIST_MEM_ENABLED) then
       plan = halo_plan_for(ssha%grid%nx, ssha%grid%ny)
    else
       plan = serial_plan_for(ssha%grid%nx, ssha%grid%ny)
    end if
    wet = c_null_ptr
    if (present(skip_land)) then
       if (skip_land) wet = wet_plan(ssha%grid)
    end if
    ! (a null wet plan: dlesm_nemolite_step_dm)
    rc = dlesm_nemolite_step_wet_dm(plan, wet, params, mg, ssha%grid%area_t_device, int(ssha%grid%nx, c_int), &
                                    int(ssha%grid%ny, c_int), tbox, ubox, vbox, obc, bc, field_device_data(un), &
                                    field_device_data(vn), field_device_data(ht), field_device_data(hu), &
                                    field_device_data(hv), field_device_data(sshn_t), field_device_data(sshn_u), &
                                    field_device_data(sshn_v), field_device_data(ssha), field_device_data(ssha_u), &
                                    field_device_data(ssha_v), field_device_data(ua), field_device_data(va), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_nemolite_step_dm: ' // dlesm_error_text())
  end subroutine invoke_nemolite_step_dm

  !> Upwind transport of up to DLESM_TRACER_MAX T-point tracers in one sweep (DESIGN.md section 6.10): c_out(k) <- c_in(k)
  !! carried by continuity's face transports of level n (un, vn, hu, hv, sshn_u, sshn_v), from the water column ht + sshn_t to
  !! ht + ssha, over the T internal region, on wet cells only.  ssha is what the time step made from the same level-n inputs.
  !! Single domain: stops on a decomposed grid (use invoke_tracer_step_dm), and when c_out and c_in differ in size.
  subroutine invoke_tracer_step(rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v)
    real(go_wp), intent(in) :: rdt
    type(r2d_field), intent(inout), target :: c_out(:), c_in(:)
    type(r2d_field), intent(inout), target :: ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v
    if (ssha%grid%decomp%ndomains > 1) &
         call gocean_stop('invoke_tracer_step: the grid is decomposed: the new tracers need a halo exchange; use ' // &
                          'invoke_tracer_step_dm')
    call tracer_step_call('invoke_tracer_step', c_null_ptr, .false., 0, rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, sshn_t, &
                          sshn_u, sshn_v)
  end subroutine invoke_tracer_step

  !> invoke_tracer_step and ONE exchange of the new tracers on a decomposed grid (dlesm_tracer_step_dm, DESIGN.md section
  !! 6.10): bit for bit invoke_tracer_step, then the halo exchange of c_out.  The flow fields and c_in need valid depth-1 halos;
  !! c_out leaves with them.  Collective.  The grid must have been decomposed with halo_width = 1 (without distributed memory
  !! the plan has no messages: invoke_tracer_step, bit for bit).
  subroutine invoke_tracer_step_dm(rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v)
    use parallel_comms_mod, only: halo_plan_for, serial_plan_for
    use parallel_utils_mod, only: DIST_MEM_ENABLED
    real(go_wp), intent(in) :: rdt
    type(r2d_field), intent(inout), target :: c_out(:), c_in(:)
    type(r2d_field), intent(inout), target :: ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v
    type(c_ptr) :: plan
    if (ssha%grid%subdomain%internal%xstart - 1 /= 1 .or. ssha%grid%subdomain%internal%ystart - 1 /= 1) &
         call gocean_stop('invoke_tracer_step_dm: the grid must be decomposed with halo_width = 1')
    if (DIST_MEM_ENABLED) then
       plan = halo_plan_for(ssha%grid%nx, ssha%grid%ny)
    else
       plan = serial_plan_for(ssha%grid%nx, ssha%grid%ny)
    end if
    call tracer_step_call('invoke_tracer_step_dm', plan, .true., 0, rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, &
                          sshn_v)
  end subroutine invoke_tracer_step_dm

  !> invoke_tracer_step with second-order limited face values (dlesm_tracer_step_muscl_f64, DESIGN.md section 6.11): the upwind
  !! cell's monotonised-central slope rebuilds what a face carries; land, open cells and cells next to land keep the upwind
  !! value.  Same arguments and rules.  Single domain: stops on a decomposed grid (use invoke_tracer_step_muscl_dm).
  subroutine invoke_tracer_step_muscl(rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v)
    real(go_wp), intent(in) :: rdt
    type(r2d_field), intent(inout), target :: c_out(:), c_in(:)
    type(r2d_field), intent(inout), target :: ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v
    if (ssha%grid%decomp%ndomains > 1) &
         call gocean_stop('invoke_tracer_step_muscl: the grid is decomposed: the new tracers need a halo exchange; use ' // &
                          'invoke_tracer_step_muscl_dm')
    call tracer_step_call('invoke_tracer_step_muscl', c_null_ptr, .false., 1, rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, &
                          sshn_t, sshn_u, sshn_v)
  end subroutine invoke_tracer_step_muscl

  !> invoke_tracer_step_muscl and ONE depth-2 exchange of the new tracers on a decomposed grid (dlesm_tracer_step_muscl_dm,
  !! DESIGN.md section 6.11).  The grid's mask and c_in need valid depth-2 halos, the flow fields depth-1 halos; c_out leaves
  !! with depth-2 halos.  Collective.  The grid must have been decomposed with halo_width = 2 (without distributed memory the
  !! plan has no messages: invoke_tracer_step_muscl, bit for bit).
  subroutine invoke_tracer_step_muscl_dm(rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v)
    use parallel_comms_mod, only: halo_plan_for, serial_plan_for
    use parallel_utils_mod, only: DIST_MEM_ENABLED
    real(go_wp), intent(in) :: rdt
    type(r2d_field), intent(inout), target :: c_out(:), c_in(:)
    type(r2d_field), intent(inout), target :: ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v
    type(c_ptr) :: plan
    if (ssha%grid%subdomain%internal%xstart - 1 /= 2 .or. ssha%grid%subdomain%internal%ystart - 1 /= 2) &
         call gocean_stop('invoke_tracer_step_muscl_dm: the grid must be decomposed with halo_width = 2')
    if (DIST_MEM_ENABLED) then
       plan = halo_plan_for(ssha%grid%nx, ssha%grid%ny)
    else
       plan = serial_plan_for(ssha%grid%nx, ssha%grid%ny)
    end if
    call tracer_step_call('invoke_tracer_step_muscl_dm', plan, .true., 1, rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, &
                          sshn_t, sshn_u, sshn_v)
  end subroutine invoke_tracer_step_muscl_dm

  !> invoke_tracer_step_muscl with time-centred face values (dlesm_tracer_step_hancock_f64, DESIGN.md section 6.12): the slope's
  !! factor 0.5 becomes 0.5 * (1 - n), n the face's Courant number in its upwind cell, 0 where n is not in [0, 1).  Same
  !! arguments and rules.  Single domain: stops on a decomposed grid (use invoke_tracer_step_hancock_dm).
  subroutine invoke_tracer_step_hancock(rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v)
    real(go_wp), intent(in) :: rdt
    type(r2d_field), intent(inout), target :: c_out(:), c_in(:)
    type(r2d_field), intent(inout), target :: ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v
    if (ssha%grid%decomp%ndomains > 1) &
         call gocean_stop('invoke_tracer_step_hancock: the grid is decomposed: the new tracers need a halo exchange; use ' // &
                          'invoke_tracer_step_hancock_dm')
    call tracer_step_call('invoke_tracer_step_hancock', c_null_ptr, .false., 2, rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, &
                          sshn_t, sshn_u, sshn_v)
  end subroutine invoke_tracer_step_hancock

  !> invoke_tracer_step_hancock and ONE depth-2 exchange of the new tracers on a decomposed grid (dlesm_tracer_step_hancock_dm,
  !! DESIGN.md section 6.12).  The grid's mask and c_in need valid depth-2 halos, the flow fields depth-1 halos; c_out leaves
  !! with depth-2 halos.  Collective.  The grid must have been decomposed with halo_width = 2 (without distributed memory the
  !! plan has no messages: invoke_tracer_step_hancock, bit for bit).
  subroutine invoke_tracer_step_hancock_dm(rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v)
    use parallel_comms_mod, only: halo_plan_for, serial_plan_for
    use parallel_utils_mod, only: DIST_MEM_ENABLED
    real(go_wp), intent(in) :: rdt
    type(r2d_field), intent(inout), target :: c_out(:), c_in(:)
    type(r2d_field), intent(inout), target :: ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v
    type(c_ptr) :: plan
    if (ssha%grid%subdomain%internal%xstart - 1 /= 2 .or. ssha%grid%subdomain%internal%ystart - 1 /= 2) &
         call gocean_stop('invoke_tracer_step_hancock_dm: the grid must be decomposed with halo_width = 2')
    if (DIST_MEM_ENABLED) then
       plan = halo_plan_for(ssha%grid%nx, ssha%grid%ny)
    else
       plan = serial_plan_for(ssha%grid%nx, ssha%grid%ny)
    end if
    call tracer_step_call('invoke_tracer_step_hancock_dm', plan, .true., 2, rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, &
                          sshn_t, sshn_u, sshn_v)
  end subroutine invoke_tracer_step_hancock_dm

  !> One coupled time step on a decomposed grid (dlesm_nemolite_coupled_step_dm, DESIGN.md section 6.13): the flow step of
  !! invoke_nemolite_step_dm and the tracer sweep of `scheme` (DLESM_TRACER_UPWIND, DLESM_TRACER_MUSCL or DLESM_TRACER_HANCOCK)
  !! with rdt = params%rdt, c_in carried to c_out by the level-n transports into the new water column, then ONE exchange of
  !! ssha, ssha_u, ssha_v, ua, va and every c_out.  Arrays of size zero: the flow step alone.  The flow inputs need valid depth-1
  !! halos, corners included; c_in depth-1 halos for the upwind scheme, c_in and the grid's mask depth-2 halos for the limited
  !! ones (exchange_mask_halos fills the mask's); every output leaves with halos of the grid's halo width.  Collective.  The
  !! grid must have been decomposed with halo_width = 1 or 2, a limited scheme needs halo_width = 2 (without distributed memory
  !! the plan has no messages: invoke_nemolite_step and the single-domain tracer wrapper, bit for bit).  ssh_bc and skip_land as
  !! invoke_nemolite_step_dm.
  subroutine invoke_nemolite_coupled_step_dm(params, scheme, c_out, c_in, ssha, ssha_u, ssha_v, ua, va, un, vn, ht, hu, hv, &
                                             sshn_t, sshn_u, sshn_v, ssh_bc, skip_land)
    use parallel_comms_mod, only: halo_plan_for, serial_plan_for
    use parallel_utils_mod, only: DIST_MEM_ENABLED
    type(c_momentum_params), intent(in) :: params
    integer, intent(in) :: scheme
    type(r2d_field), intent(inout), target :: c_out(:), c_in(:)
    type(r2d_field), intent(inout), target :: ssha, ssha_u, ssha_v, ua, va, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v
    real(go_wp), optional, intent(in) :: ssh_bc
    logical, optional, intent(in) :: skip_land
    type(c_momentum_grid) :: mg
    type(c_region) :: tbox, ubox, vbox
    type(c_ptr) :: plan, obc, wet
    type(c_ptr) :: pin(DLESM_TRACER_MAX), pout(DLESM_TRACER_MAX)
    real(c_double) :: bc
    integer(c_int) :: rc
    integer :: hw, k, n
    hw = ssha%grid%subdomain%internal%xstart - 1
    if ((hw /= 1 .and. hw /= 2) .or. ssha%grid%subdomain%internal%ystart - 1 /= hw) &
         call gocean_stop('invoke_nemolite_coupled_step_dm: the grid must be decomposed with halo_width = 1 or 2')
    if (scheme < DLESM_TRACER_UPWIND .or. scheme > DLESM_TRACER_HANCOCK) &
         call gocean_stop('invoke_nemolite_coupled_step_dm: the scheme must be DLESM_TRACER_UPWIND, _MUSCL or _HANCOCK')
    n = size(c_in)
    if (size(c_out) /= n) call gocean_stop('invoke_nemolite_coupled_step_dm: c_out and c_in differ in size')
    if (n > DLESM_TRACER_MAX) call gocean_stop('invoke_nemolite_coupled_step_dm: the number of tracers must be 0..8')
    if (hw == 1 .and. scheme /= DLESM_TRACER_UPWIND .and. n > 0) &
         call gocean_stop('invoke_nemolite_coupled_step_dm: a limited scheme reads two cells: the grid must be decomposed ' // &
                          'with halo_width = 2')
    call need_device(ssha);  call need_device(ssha_u);  call need_device(ssha_v);  call need_device(ua);  call need_device(va)
    call need_device(un);  call need_device(vn);  call need_device(ht);  call need_device(hu);  call need_device(hv)
    call need_device(sshn_t);  call need_device(sshn_u);  call need_device(sshn_v)
    pin = c_null_ptr;  pout = c_null_ptr
    do k = 1, n
       call need_device(c_in(k));  call need_device(c_out(k))
       pin(k) = field_device_data(c_in(k));  pout(k) = field_device_data(c_out(k))
    end do
    mg = momentum_grid(ssha%grid, 'invoke_nemolite_coupled_step_dm')
    tbox = c_region(ssha%internal%nx, ssha%internal%ny, ssha%internal%xstart, ssha%internal%xstop, &
                    ssha%internal%ystart, ssha%internal%ystop)
    ubox = c_region(ua%internal%nx, ua%internal%ny, ua%internal%xstart, ua%internal%xstop, &
                    ua%internal%ystart, ua%internal%ystop)
    vbox = c_region(va%internal%nx, va%internal%ny, va%internal%xstart, va%internal%xstop, &
                    va%internal%ystart, va%internal%ystop)
    obc = c_null_ptr
    bc = 0.0_c_double
    if (present(ssh_bc)) then
       obc = open_boundary(ssha%grid)
       bc = real(ssh_bc, c_double)
    end if
    if (DIST_MEM_ENABLED) then
       plan = halo_plan_for(ssha%grid%nx, ssha%grid%ny)
    else
       plan = serial_plan_for(ssha%grid%nx, ssha%grid%ny)
    end if
    wet = c_null_ptr
    if (present(skip_land)) then
       if (skip_land) wet = wet_plan(ssha%grid)
    end if
    rc = dlesm_nemolite_coupled_step_dm(plan, wet, int(scheme, c_int), params, mg, ssha%grid%area_t_device, &
                                        int(ssha%grid%nx, c_int), int(ssha%grid%ny, c_int), tbox, ubox, vbox, obc, bc, &
                                        field_device_data(un), field_device_data(vn), field_device_data(ht), &
                                        field_device_data(hu), field_device_data(hv), field_device_data(sshn_t), &
                                        field_device_data(sshn_u), field_device_data(sshn_v), field_device_data(ssha), &
                                        field_device_data(ssha_u), field_device_data(ssha_v), field_device_data(ua), &
                                        field_device_data(va), pin, pout, int(n, c_int), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_nemolite_coupled_step_dm: ' // dlesm_error_text())
  end subroutine invoke_nemolite_coupled_step_dm

  !> "May I take a tracer step with this rdt" (dlesm_tracer_courant_f64, DESIGN.md section 6.14): one read-only sweep over the
  !! level-n flow, over the T internal region with the grid's mask and area_t, that needs no ssha.  res, the same on every rank:
  !! the largest face Courant number of a wet cell exactly as invoke_tracer_step_hancock computes it, the largest outflow
  !! number, how many wet cells reach face_limit (default 0.5) and outflow_limit (default 1.0), how many hold a number that is
  !! not finite and >= 0, and how many are wet.  res%face_index / res%outflow_index are those of the owning rank -- the lowest
  !! rank (1-based, get_rank) that holds a cell with the maximum, returned in face_rank / outflow_rank (0: none, index -1) --
  !! 0-based linear in its local arrays: i = mod(index, nx) + 1, j = index / nx + 1.  Synchronous.  On a decomposed grid the
  !! flow fields need valid depth-1 halos; collective there.
  subroutine tracer_courant(rdt, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, res, face_limit, outflow_limit, face_rank, &
                            outflow_rank)
    use rank_collectives_mod, only: place, rank_total
    real(go_wp), intent(in) :: rdt
    type(r2d_field), intent(inout), target :: un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v
    type(tracer_courant_type), intent(out) :: res
    real(go_wp), optional, intent(in) :: face_limit, outflow_limit
    integer, optional, intent(out) :: face_rank, outflow_rank
    real(c_double) :: fl, ol
    integer(c_int) :: rc
    integer :: fr, orank
    fl = 0.5_c_double;  ol = 1.0_c_double
    if (present(face_limit)) fl = real(face_limit, c_double)
    if (present(outflow_limit)) ol = real(outflow_limit, c_double)
    call need_device(un);  call need_device(vn);  call need_device(ht);  call need_device(hu);  call need_device(hv)
    call need_device(sshn_t);  call need_device(sshn_u);  call need_device(sshn_v)
    call grid_to_device(sshn_t%grid)
    rc = dlesm_tracer_courant_f64(real(rdt, c_double), int(sshn_t%grid%nx, c_int), int(sshn_t%grid%ny, c_int), &
                                  int(sshn_t%internal%xstart, c_int), int(sshn_t%internal%xstop, c_int), &
                                  int(sshn_t%internal%ystart, c_int), int(sshn_t%internal%ystop, c_int), &
                                  sshn_t%grid%tmask_device, sshn_t%grid%area_t_device, field_device_data(un), &
                                  field_device_data(vn), field_device_data(hu), field_device_data(hv), field_device_data(ht), &
                                  field_device_data(sshn_t), field_device_data(sshn_u), field_device_data(sshn_v), fl, ol, &
                                  res, c_null_ptr)
    if (rc /= 0) call gocean_stop('tracer_courant: ' // dlesm_error_text())
    call place('tracer_courant', res%face_max, res%face_index, fr)
    call place('tracer_courant', res%outflow_max, res%outflow_index, orank)
    call rank_total('tracer_courant', res%face_over);  call rank_total('tracer_courant', res%outflow_over)
    call rank_total('tracer_courant', res%invalid);  call rank_total('tracer_courant', res%wet)
    if (present(face_rank)) face_rank = fr
    if (present(outflow_rank)) outflow_rank = orank
  end subroutine tracer_courant

  !> "May the flow step take this rdt" (dlesm_flow_courant_f64, DESIGN.md section 6.15): one read-only sweep over the level-n
  !! flow, over the T internal region with the grid's mask, dx_t and dy_t.  res, the same on every rank: the largest
  !! gravity-wave, advective and viscous number of a wet cell and the smallest water column, how many wet cells reach
  !! gravity_limit (default 1), advective_limit (1) and viscous_limit (0.25), how many are no deeper than depth_limit (0), how
  !! many are invalid and how many are wet.  g defaults to 9.80665 and visc to 0 -- pass the flow step's own.  The four indices
  !! are those of the owning rank -- the lowest rank (1-based, get_rank) that holds a cell with the extreme, returned in
  !! gravity_rank .. depth_rank (0: none, index -1) -- 0-based linear in its local arrays: i = mod(index, nx) + 1,
  !! j = index / nx + 1.  Synchronous.  On a decomposed grid the fields need valid depth-1 halos; collective there.
  subroutine flow_courant(rdt, un, vn, ht, sshn_t, res, g, visc, gravity_limit, advective_limit, viscous_limit, depth_limit, &
                          gravity_rank, advective_rank, viscous_rank, depth_rank)
    use rank_collectives_mod, only: place, rank_total
    real(go_wp), intent(in) :: rdt
    type(r2d_field), intent(inout), target :: un, vn, ht, sshn_t
    type(flow_courant_type), intent(out) :: res
    real(go_wp), optional, intent(in) :: g, visc, gravity_limit, advective_limit, viscous_limit, depth_limit
    integer, optional, intent(out) :: gravity_rank, advective_rank, viscous_rank, depth_rank
    real(c_double) :: gv, nu, gl, al, vl, dl, deep
    integer(c_int) :: rc
    integer :: gr, ar, vr, dr
    gv = 9.80665_c_double;  nu = 0.0_c_double
    gl = 1.0_c_double;  al = 1.0_c_double;  vl = 0.25_c_double;  dl = 0.0_c_double
    if (present(g)) gv = real(g, c_double)
    if (present(visc)) nu = real(visc, c_double)
    if (present(gravity_limit)) gl = real(gravity_limit, c_double)
    if (present(advective_limit)) al = real(advective_limit, c_double)
    if (present(viscous_limit)) vl = real(viscous_limit, c_double)
    if (present(depth_limit)) dl = real(depth_limit, c_double)
    call need_device(un);  call need_device(vn);  call need_device(ht);  call need_device(sshn_t)
    call grid_to_device(sshn_t%grid)
    rc = dlesm_flow_courant_f64(real(rdt, c_double), gv, nu, int(sshn_t%grid%nx, c_int), int(sshn_t%grid%ny, c_int), &
                                int(sshn_t%internal%xstart, c_int), int(sshn_t%internal%xstop, c_int), &
                                int(sshn_t%internal%ystart, c_int), int(sshn_t%internal%ystop, c_int), &
                                sshn_t%grid%tmask_device, sshn_t%grid%dx_t_device, sshn_t%grid%dy_t_device, &
                                field_device_data(un), field_device_data(vn), field_device_data(ht), &
                                field_device_data(sshn_t), gl, al, vl, dl, res, c_null_ptr)
    if (rc /= 0) call gocean_stop('flow_courant: ' // dlesm_error_text())
    call place('flow_courant', res%gravity_max, res%gravity_index, gr)
    call place('flow_courant', res%advective_max, res%advective_index, ar)
    call place('flow_courant', res%viscous_max, res%viscous_index, vr)
    deep = -res%depth_min                                                        ! the minimum as the maximum of -d
    call place('flow_courant', deep, res%depth_index, dr)
    res%depth_min = -deep
    call rank_total('flow_courant', res%gravity_over);  call rank_total('flow_courant', res%advective_over)
    call rank_total('flow_courant', res%viscous_over);  call rank_total('flow_courant', res%shallow)
    call rank_total('flow_courant', res%invalid);  call rank_total('flow_courant', res%wet)
    if (present(gravity_rank)) gravity_rank = gr
    if (present(advective_rank)) advective_rank = ar
    if (present(viscous_rank)) viscous_rank = vr
    if (present(depth_rank)) depth_rank = dr
  end subroutine flow_courant

  !> The model's output fields in one sweep (dlesm_flow_output_f64, DESIGN.md section 6.16): of the level-n flow, into the
  !! T-point fields given -- ssh (sshn_t itself), ut and vt (the velocities brought to the T point, a face on land carrying
  !! nothing), speed (their modulus), ke (0.5 * (ht + sshn_t) * (ut**2 + vt**2)) and vort (dv/dx - du/dy at the cell's NE
  !! corner, stored only where the cells east, north and north-east are not land).  Without weight the values are stored; with
  !! it weight * value is added to what the fields hold (a time mean over nsteps: weight = 1 / nsteps into zeroed fields).
  !! Over the T internal region with the grid's mask, dx_v and dy_u; land and open cells and every halo keep their content.
  !! Asynchronous on the default stream.  On a decomposed grid un, vn and the mask need valid depth-1 halos, corners included
  !! (exchange_mask_halos fills the mask's); nothing is exchanged and the call is not collective.
  subroutine flow_output(un, vn, ht, sshn_t, ssh, ut, vt, speed, ke, vort, weight)
    type(r2d_field), intent(inout), target :: un, vn, ht, sshn_t
    type(r2d_field), optional, intent(inout), target :: ssh, ut, vt, speed, ke, vort
    real(go_wp), optional, intent(in) :: weight
    type(c_ptr) :: out(6)
    integer(c_int) :: rc, mode
    real(c_double) :: w
    out = c_null_ptr
    if (present(ssh)) call want(ssh, 1)
    if (present(ut)) call want(ut, 2)
    if (present(vt)) call want(vt, 3)
    if (present(speed)) call want(speed, 4)
    if (present(ke)) call want(ke, 5)
    if (present(vort)) call want(vort, 6)
    mode = 0_c_int;  w = 0.0_c_double
    if (present(weight)) then
       mode = 1_c_int;  w = real(weight, c_double)
    end if
    call need_device(un);  call need_device(vn);  call need_device(ht);  call need_device(sshn_t)
    call grid_to_device(sshn_t%grid)
    rc = dlesm_flow_output_f64(mode, w, int(sshn_t%grid%nx, c_int), int(sshn_t%grid%ny, c_int), &
                               int(sshn_t%internal%xstart, c_int), int(sshn_t%internal%xstop, c_int), &
                               int(sshn_t%internal%ystart, c_int), int(sshn_t%internal%ystop, c_int), &
                               sshn_t%grid%tmask_device, sshn_t%grid%dx_v_device, sshn_t%grid%dy_u_device, &
                               field_device_data(un), field_device_data(vn), field_device_data(ht), &
                               field_device_data(sshn_t), out, c_null_ptr)
    if (rc /= 0) call gocean_stop('flow_output: ' // dlesm_error_text())
  contains
    subroutine want(f, k)
      type(r2d_field), intent(inout), target :: f
      integer, intent(in) :: k
      call need_device(f)
      out(k) = field_device_data(f)
    end subroutine want
  end subroutine flow_output

  !> A set of drifters on the device (DESIGN.md section 6.17): n particles at px, py in local index coordinates (T cell
  !! (i, j) covers [i, i+1) x [j, j+1)), all ACTIVE unless status (0 ACTIVE, 1 LEFT, 2 OPEN, 3 GROUNDED) says otherwise.
  subroutine drifters_create(set, px, py, status)
    type(drifters_type), intent(inout) :: set
    real(go_wp), intent(in), target :: px(:), py(:)
    integer(c_int), optional, intent(in), target :: status(:)
    real(c_double), allocatable, target :: x(:), y(:)
    integer(c_int), allocatable, target :: s(:)
    integer(c_int) :: rc
    type(c_ptr) :: ps
    if (c_associated(set%handle)) call drifters_free(set)
    if (size(py) /= size(px)) call gocean_stop('drifters_create: px and py differ in size')
    set%n = size(px, kind=c_long_long)
    rc = dlesm_drifters_create(set%n, set%handle)
    if (rc /= 0) call gocean_stop('drifters_create: ' // dlesm_error_text())
    allocate(x(size(px)), y(size(px)))                    ! contiguous copies, whatever section the caller passed
    x = real(px, c_double);  y = real(py, c_double)
    ps = c_null_ptr
    if (present(status)) then
       if (size(status) /= size(px)) call gocean_stop('drifters_create: px and status differ in size')
       allocate(s(size(px)))
       s = status
       ps = c_loc(s)
    end if
    rc = dlesm_drifters_put(set%handle, c_loc(x), c_loc(y), ps)
    if (rc /= 0) call gocean_stop('drifters_create: ' // dlesm_error_text())
  end subroutine drifters_create

  !> The set's positions and statuses on the host, after waiting for the device
  subroutine drifters_get(set, px, py, status)
    type(drifters_type), intent(in) :: set
    real(go_wp), intent(out) :: px(:), py(:)
    integer(c_int), intent(out) :: status(:)
    real(c_double), allocatable, target :: x(:), y(:)
    integer(c_int), allocatable, target :: s(:)
    integer(c_int) :: rc
    if (.not. c_associated(set%handle)) call gocean_stop('drifters_get: the set has not been created')
    if (size(px) /= set%n .or. size(py) /= set%n .or. size(status) /= set%n) &
         call gocean_stop('drifters_get: px, py and status hold one element per particle')
    allocate(x(set%n), y(set%n), s(set%n))
    rc = dlesm_drifters_get(set%handle, c_loc(x), c_loc(y), c_loc(s))
    if (rc /= 0) call gocean_stop('drifters_get: ' // dlesm_error_text())
    px = real(x, go_wp);  py = real(y, go_wp);  status = s
  end subroutine drifters_get

  subroutine drifters_free(set)
    type(drifters_type), intent(inout) :: set
    integer(c_int) :: rc
    if (c_associated(set%handle)) then
       rc = dlesm_drifters_destroy(set%handle)
       if (rc /= 0) call gocean_stop('drifters_free: ' // dlesm_error_text())
    end if
    set%handle = c_null_ptr
    set%n = 0
  end subroutine drifters_free

  !> What drifter_step, dispersal_step and random_walk do before their call, stopping under the caller's name `who`: the set
  !! has been created, kh_t (where given) is a T-point field of un's grid, the fields and the grid are on the device; box
  !! becomes the T internal region of un's grid.
  subroutine particle_step_box(who, set, un, vn, box, kh_t)
    character(len=*), intent(in) :: who
    type(drifters_type), intent(in) :: set
    type(r2d_field), intent(inout), target :: un, vn
    type(c_region), intent(out) :: box
    type(r2d_field), intent(inout), target, optional :: kh_t
    type(c_region) :: sub, whole
    integer(c_int) :: rc
    if (.not. c_associated(set%handle)) call gocean_stop(who // ': the set has not been created')
    if (present(kh_t)) then
       if (.not. associated(kh_t%grid, un%grid) .or. kh_t%defined_on /= GO_T_POINTS) &
            call gocean_stop(who // ': kh_t is a T-point field of the grid of un')
    end if
    call need_device(un);  call need_device(vn)
    if (present(kh_t)) call need_device(kh_t)
    call grid_to_device(un%grid)
    associate (g => un%grid, s => un%grid%subdomain%internal)
      sub = c_region(s%nx, s%ny, s%xstart, s%xstop, s%ystart, s%ystop)
      rc = dlesm_field_bounds(int(GO_T_POINTS, c_int), int(g%offset, c_int), int(g%boundary_conditions(1), c_int), &
                              int(g%boundary_conditions(2), c_int), sub, int(g%nx, c_int), int(g%ny, c_int), box, whole)
    end associate
    if (rc /= 0) call gocean_stop(who // ': ' // dlesm_error_text())
  end subroutine particle_step_box

  !> Carry the set through the level-n flow (dlesm_drifter_step_f64, DESIGN.md section 6.17): nsub substeps of h seconds by
  !! the midpoint rule, in place, over the T internal region of un's grid with the grid's mask, dx_t and dy_t.  A particle
  !! that leaves the region becomes LEFT and one that reaches an open cell OPEN, both at their new position; one whose move
  !! would end on land becomes GROUNDED at its last wet position.  Asynchronous on the default stream.  On a decomposed grid
  !! un, vn and the mask need valid depth-1 halos; nothing is exchanged and the call is not collective.
  subroutine drifter_step(set, h, nsub, un, vn)
    type(drifters_type), intent(inout) :: set
    real(go_wp), intent(in) :: h
    integer, intent(in) :: nsub
    type(r2d_field), intent(inout), target :: un, vn
    type(c_region) :: box
    type(c_ptr) :: px, py, status
    integer(c_long_long) :: n
    integer(c_int) :: rc
    call particle_step_box('drifter_step', set, un, vn, box)
    rc = dlesm_drifters_arrays(set%handle, n, px, py, status)
    if (rc /= 0) call gocean_stop('drifter_step: ' // dlesm_error_text())
    associate (g => un%grid)
      rc = dlesm_drifter_step_f64(real(h, c_double), int(nsub, c_int), int(g%nx, c_int), int(g%ny, c_int), box%xstart, &
                                  box%xstop, box%ystart, box%ystop, g%tmask_device, g%dx_t_device, g%dy_t_device, &
                                  field_device_data(un), field_device_data(vn), n, px, py, status, c_null_ptr)
    end associate
    if (rc /= 0) call gocean_stop('drifter_step: ' // dlesm_error_text())
  end subroutine drifter_step

  !> drifter_step with random-walk diffusion (dlesm_dispersal_step_set, DESIGN.md section 6.20): every substep adds a kick,
  !! uniform with variance 2 kh |h| per axis (kh: a constant horizontal diffusivity in m2/s), drawn from Philox4x32-10 with
  !! the seed as key and (the particle's index at drifters_create, tick + substep) as counter; a kick that would end on land
  !! is rejected.  seed: any 64 bits; tick: the substeps taken so far (>= 0), which the caller advances by nsub from call to
  !! call.  A particle keeps its random stream through particle_sort.  The region, the mask, the metrics and the statuses are
  !! drifter_step's.  Asynchronous on the default stream; nothing is exchanged and the call is not collective.
  subroutine dispersal_step(set, h, nsub, kh, seed, tick, un, vn)
    type(drifters_type), intent(inout) :: set
    real(go_wp), intent(in) :: h
    integer, intent(in) :: nsub
    real(go_wp), intent(in) :: kh
    integer(c_long_long), intent(in) :: seed, tick
    type(r2d_field), intent(inout), target :: un, vn
    type(c_region) :: box
    integer(c_int) :: rc
    call particle_step_box('dispersal_step', set, un, vn, box)
    associate (g => un%grid)
      rc = dlesm_dispersal_step_set(set%handle, real(h, c_double), int(nsub, c_int), real(kh, c_double), seed, tick, &
                                    c_null_ptr, int(g%nx, c_int), int(g%ny, c_int), box%xstart, box%xstop, box%ystart, &
                                    box%ystop, g%tmask_device, g%dx_t_device, g%dy_t_device, field_device_data(un), &
                                    field_device_data(vn), c_null_ptr)
    end associate
    if (rc /= 0) call gocean_stop('dispersal_step: ' // dlesm_error_text())
  end subroutine dispersal_step

  !> dispersal_step in a diffusivity that varies in space (dlesm_random_walk_set, DESIGN.md section 6.22): kh_t is a T-point
  !! field of un's grid in m2/s, finite and >= 0 wherever the mask is not 0.  Per substep and axis a particle drifts by
  !! |h| dK/dx (Visser's correction, without which particles collect where mixing is weak) and takes a kick sized by K half a
  !! drift ahead; a constant field gives dispersal_step's bits.  seed, tick, the region, the mask, the metrics, the statuses
  !! and the random streams through particle_sort are dispersal_step's.  On a decomposed grid kh_t needs valid depth-1 halos,
  !! like un, vn and the mask.  Asynchronous on the default stream; nothing is exchanged and the call is not collective.
  subroutine random_walk(set, h, nsub, kh_t, seed, tick, un, vn)
    type(drifters_type), intent(inout) :: set
    real(go_wp), intent(in) :: h
    integer, intent(in) :: nsub
    type(r2d_field), intent(inout), target :: kh_t
    integer(c_long_long), intent(in) :: seed, tick
    type(r2d_field), intent(inout), target :: un, vn
    type(c_region) :: box
    integer(c_int) :: rc
    call particle_step_box('random_walk', set, un, vn, box, kh_t)
    associate (g => un%grid)
      rc = dlesm_random_walk_set(set%handle, real(h, c_double), int(nsub, c_int), field_device_data(kh_t), seed, tick, &
                                 c_null_ptr, int(g%nx, c_int), int(g%ny, c_int), box%xstart, box%xstop, box%ystart, &
                                 box%ystop, g%tmask_device, g%dx_t_device, g%dy_t_device, field_device_data(un), &
                                 field_device_data(vn), c_null_ptr)
    end associate
    if (rc /= 0) call gocean_stop('random_walk: ' // dlesm_error_text())
  end subroutine random_walk

  !> Bring the set into cell order (dlesm_particle_sort_set, DESIGN.md section 6.18): the particles that are ACTIVE and inside
  !! the T internal region of un's grid -- the box drifter_step uses -- come first, in the row-major order of their cells and,
  !! within a cell, in their old order; every other particle follows in its old order.  drifter_step then reads the flow
  !! nearly in order.  Asynchronous on the default stream; the first call on a set allocates its second buffers.
  subroutine particle_sort(set, un)
    type(drifters_type), intent(inout) :: set
    type(r2d_field), intent(in) :: un
    type(c_region) :: sub, box, whole
    integer(c_int) :: rc
    if (.not. c_associated(set%handle)) call gocean_stop('particle_sort: the set has not been created')
    associate (g => un%grid)
      associate (s => g%subdomain%internal)
        sub = c_region(s%nx, s%ny, s%xstart, s%xstop, s%ystart, s%ystop)
      end associate
      rc = dlesm_field_bounds(int(GO_T_POINTS, c_int), int(g%offset, c_int), int(g%boundary_conditions(1), c_int), &
                              int(g%boundary_conditions(2), c_int), sub, int(g%nx, c_int), int(g%ny, c_int), box, whole)
    end associate
    if (rc /= 0) call gocean_stop('particle_sort: ' // dlesm_error_text())
    rc = dlesm_particle_sort_set(set%handle, box%xstart, box%xstop, box%ystart, box%ystop, c_null_ptr)
    if (rc /= 0) call gocean_stop('particle_sort: ' // dlesm_error_text())
  end subroutine particle_sort

  !> Where the set's particles came from, after waiting for the device: origin(k) is the index (1-based), in the arrays
  !! drifters_create was given, of the particle that drifters_get now returns in slot k; nlive is the number of particles the
  !! last particle_sort put in front (-1 before the first sort).
  subroutine particle_origin(set, origin, nlive)
    type(drifters_type), intent(in) :: set
    integer, intent(out) :: origin(:)
    integer, intent(out) :: nlive
    integer(c_int), allocatable, target :: o(:)
    integer(c_long_long) :: live
    integer(c_int) :: rc
    if (.not. c_associated(set%handle)) call gocean_stop('particle_origin: the set has not been created')
    if (size(origin) /= set%n) call gocean_stop('particle_origin: origin holds one element per particle')
    allocate(o(set%n))
    rc = dlesm_particle_set_origin(set%handle, c_loc(o), live)
    if (rc /= 0) call gocean_stop('particle_origin: ' // dlesm_error_text())
    origin = int(o) + 1
    nlive = int(live)
  end subroutine particle_origin

  !> The set's particles per cell (dlesm_cell_bin_set, DESIGN.md section 6.19) into the T-point field cnt, over its internal
  !! region -- the box drifter_step and particle_sort use: the particles that are ACTIVE and inside it are counted, exactly.
  !! mode 0 (the default) stores alpha * count in every cell of the region, mode 1 adds alpha * count to the cells that hold
  !! a particle (alpha = dt into a zeroed field: an exposure); alpha defaults to 1.  The particles are not moved.
  !! Asynchronous on the default stream; the first call on a set allocates its buffers.
  subroutine cell_bin(set, cnt, mode, alpha)
    type(drifters_type), intent(inout) :: set
    type(r2d_field), intent(inout), target :: cnt
    integer, optional, intent(in) :: mode
    real(go_wp), optional, intent(in) :: alpha
    integer(c_int) :: rc, m
    real(c_double) :: a
    if (.not. c_associated(set%handle)) call gocean_stop('cell_bin: the set has not been created')
    if (cnt%defined_on /= GO_T_POINTS) call gocean_stop('cell_bin: cnt is a field at T points')
    m = 0_c_int;  a = 1.0_c_double
    if (present(mode)) m = int(mode, c_int)
    if (present(alpha)) a = real(alpha, c_double)
    call need_device(cnt)
    rc = dlesm_cell_bin_set(set%handle, m, a, int(cnt%grid%nx, c_int), int(cnt%grid%ny, c_int), &
                            int(cnt%internal%xstart, c_int), int(cnt%internal%xstop, c_int), &
                            int(cnt%internal%ystart, c_int), int(cnt%internal%ystop, c_int), field_device_data(cnt), c_null_ptr)
    if (rc /= 0) call gocean_stop('cell_bin: ' // dlesm_error_text())
  end subroutine cell_bin

  ! the call the six tracer wrappers make (dm: the distributed entry with `plan`; scheme: 0 the upwind entries, 1 the limited
  ! scheme's, 2 the time-centred limited scheme's)
  subroutine tracer_step_call(who, plan, dm, scheme, rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v)
    character(len=*), intent(in) :: who
    type(c_ptr), intent(in) :: plan
    logical, intent(in) :: dm
    integer, intent(in) :: scheme
    real(go_wp), intent(in) :: rdt
    type(r2d_field), intent(inout), target :: c_out(:), c_in(:)
    type(r2d_field), intent(inout), target :: ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v
    type(c_ptr) :: pin(DLESM_TRACER_MAX), pout(DLESM_TRACER_MAX)
    integer :: k, n
    integer(c_int) :: rc
    n = size(c_in)
    if (size(c_out) /= n) call gocean_stop(who // ': c_out and c_in differ in size')
    if (n < 1 .or. n > DLESM_TRACER_MAX) call gocean_stop(who // ': the number of tracers must be 1..8')
    call need_device(ssha);  call need_device(un);  call need_device(vn);  call need_device(ht);  call need_device(hu)
    call need_device(hv);  call need_device(sshn_t);  call need_device(sshn_u);  call need_device(sshn_v)
    pin = c_null_ptr;  pout = c_null_ptr
    do k = 1, n
       call need_device(c_in(k));  call need_device(c_out(k))
       pin(k) = field_device_data(c_in(k));  pout(k) = field_device_data(c_out(k))
    end do
    call grid_to_device(ssha%grid)
    if (dm .and. scheme == 2) then
       rc = dlesm_tracer_step_hancock_dm(plan, real(rdt, c_double), int(ssha%grid%nx, c_int), int(ssha%grid%ny, c_int), &
                                         int(ssha%internal%xstart, c_int), int(ssha%internal%xstop, c_int), &
                                         int(ssha%internal%ystart, c_int), int(ssha%internal%ystop, c_int), &
                                         ssha%grid%tmask_device, ssha%grid%area_t_device, field_device_data(un), &
                                         field_device_data(vn), field_device_data(hu), field_device_data(hv), field_device_data(ht), &
                                         field_device_data(sshn_t), field_device_data(sshn_u), field_device_data(sshn_v), &
                                         field_device_data(ssha), pin, pout, int(n, c_int), c_null_ptr)
    else if (dm .and. scheme == 1) then
       rc = dlesm_tracer_step_muscl_dm(plan, real(rdt, c_double), int(ssha%grid%nx, c_int), int(ssha%grid%ny, c_int), &
                                       int(ssha%internal%xstart, c_int), int(ssha%internal%xstop, c_int), &
                                       int(ssha%internal%ystart, c_int), int(ssha%internal%ystop, c_int), &
                                       ssha%grid%tmask_device, ssha%grid%area_t_device, field_device_data(un), &
                                       field_device_data(vn), field_device_data(hu), field_device_data(hv), field_device_data(ht), &
                                       field_device_data(sshn_t), field_device_data(sshn_u), field_device_data(sshn_v), &
                                       field_device_data(ssha), pin, pout, int(n, c_int), c_null_ptr)
    else if (dm) then
       rc = dlesm_tracer_step_dm(plan, real(rdt, c_double), int(ssha%grid%nx, c_int), int(ssha%grid%ny, c_int), &
                                 int(ssha%internal%xstart, c_int), int(ssha%internal%xstop, c_int), &
                                 int(ssha%internal%ystart, c_int), int(ssha%internal%ystop, c_int), &
                                 ssha%grid%tmask_device, ssha%grid%area_t_device, field_device_data(un), &
                                 field_device_data(vn), field_device_data(hu), field_device_data(hv), field_device_data(ht), &
                                 field_device_data(sshn_t), field_device_data(sshn_u), field_device_data(sshn_v), &
                                 field_device_data(ssha), pin, pout, int(n, c_int), c_null_ptr)
    else if (scheme == 2) then
       rc = dlesm_tracer_step_hancock_f64(real(rdt, c_double), int(ssha%grid%nx, c_int), int(ssha%grid%ny, c_int), &
                                          int(ssha%internal%xstart, c_int), int(ssha%internal%xstop, c_int), &
                                          int(ssha%internal%ystart, c_int), int(ssha%internal%ystop, c_int), &
                                          ssha%grid%tmask_device, ssha%grid%area_t_device, field_device_data(un), &
                                          field_device_data(vn), field_device_data(hu), field_device_data(hv), field_device_data(ht), &
                                          field_device_data(sshn_t), field_device_data(sshn_u), field_device_data(sshn_v), &
                                          field_device_data(ssha), pin, pout, int(n, c_int), c_null_ptr)
    else if (scheme == 1) then
       rc = dlesm_tracer_step_muscl_f64(real(rdt, c_double), int(ssha%grid%nx, c_int), int(ssha%grid%ny, c_int), &
                                        int(ssha%internal%xstart, c_int), int(ssha%internal%xstop, c_int), &
                                        int(ssha%internal%ystart, c_int), int(ssha%internal%ystop, c_int), &
                                        ssha%grid%tmask_device, ssha%grid%area_t_device, field_device_data(un), &
                                        field_device_data(vn), field_device_data(hu), field_device_data(hv), field_device_data(ht), &
                                        field_device_data(sshn_t), field_device_data(sshn_u), field_device_data(sshn_v), &
                                        field_device_data(ssha), pin, pout, int(n, c_int), c_null_ptr)
    else
       rc = dlesm_tracer_step_f64(real(rdt, c_double), int(ssha%grid%nx, c_int), int(ssha%grid%ny, c_int), &
                                  int(ssha%internal%xstart, c_int), int(ssha%internal%xstop, c_int), &
                                  int(ssha%internal%ystart, c_int), int(ssha%internal%ystop, c_int), &
                                  ssha%grid%tmask_device, ssha%grid%area_t_device, field_device_data(un), &
                                  field_device_data(vn), field_device_data(hu), field_device_data(hv), field_device_data(ht), &
                                  field_device_data(sshn_t), field_device_data(sshn_u), field_device_data(sshn_v), &
                                  field_device_data(ssha), pin, pout, int(n, c_int), c_null_ptr)
    end if
    if (rc /= 0) call gocean_stop(who // ': ' // dlesm_error_text())
  end subroutine tracer_step_call

  !> Optional planning call (once per field geometry, outside the time loop): lets the library time
  !! its launch shapes for invoke_jacobi5 / invoke_jacobi5_dm on these fields and keep the fastest.
  !! `out` receives one valid step of `in`; results never depend on the shape.
  subroutine plan_jacobi5(out, in)
    use parallel_utils_mod, only: DIST_MEM_ENABLED
    type(r2d_field), intent(inout), target :: out, in
    integer(c_int) :: rc, shrink
    call need_device(in);  call need_device(out)
    shrink = 0
    if (DIST_MEM_ENABLED) shrink = 1         ! the distributed step's interior box
    rc = dlesm_stencil5_autotune_f64(field_device_data(in), field_device_data(out), &
                                     int(out%grid%nx, c_int), int(out%grid%ny, c_int), &
                                     int(out%internal%xstart + shrink, c_int), int(out%internal%xstop - shrink, c_int), &
                                     int(out%internal%ystart + shrink, c_int), int(out%internal%ystop - shrink, c_int), &
                                     c_null_ptr)
    if (rc /= 0) call gocean_stop('plan_jacobi5: ' // dlesm_error_text())
  end subroutine plan_jacobi5

  !> Distributed Jacobi step: `in` must have valid halos; on return (asynchronously) `out`
  !! holds the update AND its halos, the exchange having run behind the interior sweep.
  subroutine invoke_jacobi5_dm(out, in)
    use parallel_comms_mod, only: halo_plan_for
    use parallel_utils_mod, only: DIST_MEM_ENABLED
    type(r2d_field), intent(inout), target :: out, in
    integer(c_int) :: rc
    if (.not. DIST_MEM_ENABLED) then
       call invoke_jacobi5(out, in)
       return
    end if
    call need_device(in);  call need_device(out)
    rc = dlesm_jacobi5_step_dm(halo_plan_for(out%grid%nx, out%grid%ny), field_device_data(in), &
                               field_device_data(out), int(out%grid%nx, c_int), int(out%grid%ny, c_int), &
                               int(out%internal%xstart, c_int), int(out%internal%xstop, c_int), &
                               int(out%internal%ystart, c_int), int(out%internal%ystop, c_int), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_jacobi5_dm: ' // dlesm_error_text())
  end subroutine invoke_jacobi5_dm

  !> The same step for a time loop of such steps: returns with the exchange of `out` in flight;
  !! the next invoke_jacobi5_dm_pipelined on this grid waits for it on the device, any other library
  !! call on the grid's plan joins it first, and halo_join(grid) orders everything else behind it.
  subroutine invoke_jacobi5_dm_pipelined(out, in)
    use parallel_comms_mod, only: halo_plan_for
    use parallel_utils_mod, only: DIST_MEM_ENABLED
    type(r2d_field), intent(inout), target :: out, in
    integer(c_int) :: rc
    if (.not. DIST_MEM_ENABLED) then
       call invoke_jacobi5(out, in)
       return
    end if
    call need_device(in);  call need_device(out)
    rc = dlesm_jacobi5_step_dm_pipelined(halo_plan_for(out%grid%nx, out%grid%ny), field_device_data(in), &
                                         field_device_data(out), int(out%grid%nx, c_int), &
                                         int(out%grid%ny, c_int), int(out%internal%xstart, c_int), &
                                         int(out%internal%xstop, c_int), int(out%internal%ystart, c_int), &
                                         int(out%internal%ystop, c_int), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_jacobi5_dm_pipelined: ' // dlesm_error_text())
  end subroutine invoke_jacobi5_dm_pipelined

  !> The step of invoke_jacobi5 (the same `out`, bit for bit) that also returns how far it moved the field over
  !! out%internal on all ranks: max|out - in| (norm = 'max') or sqrt(SUM (out - in)**2) (norm = 'l2') -- what a solver
  !! checks every few steps to know when to stop.  Synchronous.  Distributed: joins a pipelined step's exchange first and
  !! leaves `out` with its depth-1 halos exchanged, as invoke_jacobi5_dm.
  function invoke_jacobi5_residual(out, in, norm) result(r)
    use parallel_comms_mod, only: halo_plan_for
    use parallel_utils_mod, only: DIST_MEM_ENABLED
    use rank_collectives_mod, only: rank_max, rank_sum
    type(r2d_field), intent(inout), target :: out, in
    character(len=*), intent(in) :: norm
    real(go_wp) :: r
    type(c_ptr), save :: dres = c_null_ptr          ! one device double, kept
    real(c_double), target :: val
    integer(c_int) :: rc, code
    select case (norm)
    case ('max')
       code = DLESM_NORM_MAX
    case ('l2')
       code = DLESM_NORM_SUMSQ
    case default
       call gocean_stop("invoke_jacobi5_residual: norm '" // norm // "' is not 'max' or 'l2'")
    end select
    call need_device(in);  call need_device(out)
    if (DIST_MEM_ENABLED) then
       rc = dlesm_halo_plan_join(halo_plan_for(out%grid%nx, out%grid%ny), c_null_ptr)
       if (rc /= 0) call gocean_stop('invoke_jacobi5_residual: ' // dlesm_error_text())
    end if
    if (.not. c_associated(dres)) then
       if (hipMalloc(dres, int(c_sizeof(val), c_size_t)) /= 0) call gocean_stop('invoke_jacobi5_residual: hipMalloc failed')
    end if
    rc = dlesm_stencil5_resid_f64(field_device_data(in), field_device_data(out), &
                                  int(out%grid%nx, c_int), int(out%grid%ny, c_int), &
                                  int(out%internal%xstart, c_int), int(out%internal%xstop, c_int), &
                                  int(out%internal%ystart, c_int), int(out%internal%ystop, c_int), code, dres, c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_jacobi5_residual: ' // dlesm_error_text())
    if (DIST_MEM_ENABLED) call out%halo_exchange(1)
    ! (hipMemcpy to pageable memory waits for the null stream, which the sweep and the exchange are on)
    if (hipMemcpy(c_loc(val), dres, int(c_sizeof(val), c_size_t), 2_c_int) /= 0) &
         call gocean_stop('invoke_jacobi5_residual: copy of the result failed')
    if (code == DLESM_NORM_MAX) then
       call rank_max('invoke_jacobi5_residual', val)
    else
       call rank_sum('invoke_jacobi5_residual', val)
       val = sqrt(val)
    end if
    r = val
  end function invoke_jacobi5_residual

  !> COLLECTIVE, once per grid: connect the grid's message plan to the neighbours' mailboxes.  From then on
  !! invoke_jacobi5_dm / invoke_jacobi5_dm_pipelined exchange by storing straight into the neighbours' memory over
  !! xGMI (the frame workgroups of the step launch are the exchange) instead of through an RCCL group per step --
  !! what MPI_Isend/Irecv/Waitany do per strip in the reference (parallel_comms_mod.f90:1601-1750).  Same results.
  !! nfields (default 1): 3 also takes the distributed shallow-water steps through the mailboxes.
  subroutine halo_connect_peers(grid, nfields)
    use parallel_comms_mod, only: halo_plan_for
    use parallel_utils_mod, only: DIST_MEM_ENABLED
    type(grid_type), intent(in) :: grid
    integer, intent(in), optional :: nfields
    integer(c_int) :: rc, nf
    if (.not. DIST_MEM_ENABLED) return
    if (dlesm_halo_plan_peer_connected(halo_plan_for(grid%nx, grid%ny)) /= 0) return
    nf = 1
    if (present(nfields)) nf = int(nfields, c_int)
    rc = dlesm_halo_plan_peer_connect_rccl(halo_plan_for(grid%nx, grid%ny), nf)
    if (rc /= 0) call gocean_stop('halo_connect_peers: ' // dlesm_error_text())
  end subroutine halo_connect_peers

  subroutine halo_join(grid)
    use parallel_comms_mod, only: halo_plan_for
    use parallel_utils_mod, only: DIST_MEM_ENABLED
    type(grid_type), intent(in) :: grid
    integer(c_int) :: rc
    if (.not. DIST_MEM_ENABLED) return
    rc = dlesm_halo_plan_join(halo_plan_for(grid%nx, grid%ny), c_null_ptr)
    if (rc /= 0) call gocean_stop('halo_join: ' // dlesm_error_text())
  end subroutine halo_join

  !> nsteps (2..8) Jacobi time steps in one sweep (temporal blocking).  Serial / one tile: the
  !! boundary ring of `in` stays fixed through all steps.  Distributed (grid decomposed with
  !! halo_width = nsteps): one depth-nsteps halo exchange per call, hidden behind the interior;
  !! `in` must hold valid depth-nsteps halos and `out` leaves with them.  Bit-identical to nsteps
  !! calls of invoke_jacobi5 (+ halo exchanges).
  subroutine invoke_jacobi5_multi(out, in, nsteps)
    use parallel_comms_mod, only: halo_plan_for
    use parallel_utils_mod, only: DIST_MEM_ENABLED
    type(r2d_field), intent(inout), target :: out, in
    integer, intent(in) :: nsteps
    integer(c_int) :: rc
    call need_device(in);  call need_device(out)
    associate (b => out%internal)
      if (DIST_MEM_ENABLED) then
         rc = dlesm_jacobi5_multi_step_dm(halo_plan_for(out%grid%nx, out%grid%ny), field_device_data(in), &
                                          field_device_data(out), int(out%grid%nx, c_int), &
                                          int(out%grid%ny, c_int), int(nsteps, c_int), int(b%xstart, c_int), &
                                          int(b%xstop, c_int), int(b%ystart, c_int), int(b%ystop, c_int), &
                                          c_null_ptr)
      else
         rc = dlesm_stencil5_multi_f64(field_device_data(in), field_device_data(out), &
                                       int(out%grid%nx, c_int), int(out%grid%ny, c_int), int(nsteps, c_int), &
                                       int(b%xstart, c_int), int(b%xstop, c_int), int(b%ystart, c_int), &
                                       int(b%ystop, c_int), int(b%xstart, c_int), int(b%xstop, c_int), &
                                       int(b%ystart, c_int), int(b%ystop, c_int), 0_c_int, 0_c_int, 0_c_int, &
                                       0_c_int, c_null_ptr)
      end if
    end associate
    if (rc /= 0) call gocean_stop('invoke_jacobi5_multi: ' // dlesm_error_text())
  end subroutine invoke_jacobi5_multi

  !> Constants of the shallow-water step; tdt = 2*dt (leapfrog)
  function shallow_params(dx, dy, dt) result(p)
    real(go_wp), intent(in) :: dx, dy, dt
    type(c_sw_params) :: p
    real(go_wp) :: tdt
    tdt = dt + dt
    p%fsdx = 4.0_go_wp / dx;  p%fsdy = 4.0_go_wp / dy
    p%tdts8 = tdt / 8.0_go_wp
    p%tdtsdx = tdt / dx;  p%tdtsdy = tdt / dy
  end function shallow_params

  subroutine invoke_shallow_step(prm, u, v, p, uold, vold, pold, unew, vnew, pnew)
    type(c_sw_params), intent(in) :: prm
    type(r2d_field), intent(inout), target :: u, v, p, uold, vold, pold, unew, vnew, pnew
    integer(c_int) :: rc
    call need_device(u);  call need_device(v);  call need_device(p)
    call need_device(uold);  call need_device(vold);  call need_device(pold)
    call need_device(unew);  call need_device(vnew);  call need_device(pnew)
    rc = dlesm_shallow_step_f64(prm, int(p%grid%nx, c_int), int(p%grid%ny, c_int), &
                                int(p%internal%xstart, c_int), int(p%internal%xstop, c_int), &
                                int(p%internal%ystart, c_int), int(p%internal%ystop, c_int), &
                                field_device_data(u), field_device_data(v), field_device_data(p), &
                                field_device_data(uold), field_device_data(vold), field_device_data(pold), &
                                field_device_data(unew), field_device_data(vnew), field_device_data(pnew), &
                                c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_shallow_step: ' // dlesm_error_text())
  end subroutine invoke_shallow_step

  !> The SW-offset form (the staggering of the GOcean `shallow` benchmark; with periodic boundaries the
  !! only configuration the reference supports for it, serially).  u, v, p must hold valid periodic
  !! halos; follow it with invoke_periodic_halos on the three new fields.
  subroutine invoke_shallow_step_sw(prm, u, v, p, uold, vold, pold, unew, vnew, pnew)
    type(c_sw_params), intent(in) :: prm
    type(r2d_field), intent(inout), target :: u, v, p, uold, vold, pold, unew, vnew, pnew
    integer(c_int) :: rc
    call need_device(u);  call need_device(v);  call need_device(p)
    call need_device(uold);  call need_device(vold);  call need_device(pold)
    call need_device(unew);  call need_device(vnew);  call need_device(pnew)
    rc = dlesm_shallow_step_sw_f64(prm, int(p%grid%nx, c_int), int(p%grid%ny, c_int), &
                                   int(p%internal%xstart, c_int), int(p%internal%xstop, c_int), &
                                   int(p%internal%ystart, c_int), int(p%internal%ystop, c_int), &
                                   field_device_data(u), field_device_data(v), field_device_data(p), &
                                   field_device_data(uold), field_device_data(vold), field_device_data(pold), &
                                   field_device_data(unew), field_device_data(vnew), field_device_data(pnew), &
                                   c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_shallow_step_sw: ' // dlesm_error_text())
  end subroutine invoke_shallow_step_sw

  !> invoke_shallow_step_sw over the internal region AND the periodic copies of the three new fields, in ONE launch:
  !! the step's edge tiles store the periodic images themselves (== invoke_shallow_step_sw followed by
  !! invoke_periodic_halos of unew, vnew, pnew, bit for bit)
  subroutine invoke_shallow_step_sw_periodic(prm, u, v, p, uold, vold, pold, unew, vnew, pnew)
    type(c_sw_params), intent(in) :: prm
    type(r2d_field), intent(inout), target :: u, v, p, uold, vold, pold, unew, vnew, pnew
    type(c_region) :: cint
    integer(c_int) :: rc
    call need_device(u);  call need_device(v);  call need_device(p)
    call need_device(uold);  call need_device(vold);  call need_device(pold)
    call need_device(unew);  call need_device(vnew);  call need_device(pnew)
    associate (it => p%internal)
      cint = c_region(it%nx, it%ny, it%xstart, it%xstop, it%ystart, it%ystop)
    end associate
    rc = dlesm_shallow_step_sw_periodic_f64(prm, int(p%grid%nx, c_int), int(p%grid%ny, c_int), cint, &
                                            int(p%grid%boundary_conditions(1), c_int), &
                                            int(p%grid%boundary_conditions(2), c_int), &
                                            field_device_data(u), field_device_data(v), field_device_data(p), &
                                            field_device_data(uold), field_device_data(vold), field_device_data(pold), &
                                            field_device_data(unew), field_device_data(vnew), field_device_data(pnew), &
                                            c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_shallow_step_sw_periodic: ' // dlesm_error_text())
  end subroutine invoke_shallow_step_sw_periodic

  !> One WHOLE time step of the GOcean leapfrog in one launch (NE offset): the u/v/h update and the Asselin filter of the
  !! old level (time_smooth) in place -- == invoke_shallow_step followed by invoke_time_smooth of u, v and p, bit for bit, at
  !! 96 B/cell instead of 168.  Afterwards rotate u <- unew (uold already holds the filtered u).
  subroutine invoke_shallow_step_smooth(prm, alpha, u, v, p, uold, vold, pold, unew, vnew, pnew)
    type(c_sw_params), intent(in) :: prm
    real(go_wp), intent(in) :: alpha
    type(r2d_field), intent(inout), target :: u, v, p, uold, vold, pold, unew, vnew, pnew
    integer(c_int) :: rc
    call need_device(u);  call need_device(v);  call need_device(p)
    call need_device(uold);  call need_device(vold);  call need_device(pold)
    call need_device(unew);  call need_device(vnew);  call need_device(pnew)
    rc = dlesm_shallow_step_smooth_f64(prm, alpha, int(p%grid%nx, c_int), int(p%grid%ny, c_int), &
                                       int(p%internal%xstart, c_int), int(p%internal%xstop, c_int), &
                                       int(p%internal%ystart, c_int), int(p%internal%ystop, c_int), &
                                       field_device_data(u), field_device_data(v), field_device_data(p), &
                                       field_device_data(uold), field_device_data(vold), field_device_data(pold), &
                                       field_device_data(unew), field_device_data(vnew), field_device_data(pnew), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_shallow_step_smooth: ' // dlesm_error_text())
  end subroutine invoke_shallow_step_smooth

  !> TWO leapfrog steps in one launch (NE offset, fixed boundary ring): level n+1 into unew, vnew, pnew and level n+2 into
  !! unew2, vnew2, pnew2 -- == invoke_shallow_step(prm, u, v, p, uold, vold, pold, unew, vnew, pnew) followed by
  !! invoke_shallow_step(prm, unew, vnew, pnew, u, v, p, unew2, vnew2, pnew2), bit for bit, at 48 instead of 72 B/cell/step.
  !! Twelve distinct fields; afterwards rotate (cur, old, new1, new2) <- (new2, new1, old, cur).
  subroutine invoke_shallow_step_x2(prm, u, v, p, uold, vold, pold, unew, vnew, pnew, unew2, vnew2, pnew2)
    type(c_sw_params), intent(in) :: prm
    type(r2d_field), intent(inout), target :: u, v, p, uold, vold, pold, unew, vnew, pnew, unew2, vnew2, pnew2
    integer(c_int) :: rc
    call need_device(u);  call need_device(v);  call need_device(p)
    call need_device(uold);  call need_device(vold);  call need_device(pold)
    call need_device(unew);  call need_device(vnew);  call need_device(pnew)
    call need_device(unew2);  call need_device(vnew2);  call need_device(pnew2)
    rc = dlesm_shallow_step_x2_f64(prm, int(p%grid%nx, c_int), int(p%grid%ny, c_int), &
                                   int(p%internal%xstart, c_int), int(p%internal%xstop, c_int), &
                                   int(p%internal%ystart, c_int), int(p%internal%ystop, c_int), &
                                   field_device_data(u), field_device_data(v), field_device_data(p), &
                                   field_device_data(uold), field_device_data(vold), field_device_data(pold), &
                                   field_device_data(unew), field_device_data(vnew), field_device_data(pnew), &
                                   field_device_data(unew2), field_device_data(vnew2), field_device_data(pnew2), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_shallow_step_x2: ' // dlesm_error_text())
  end subroutine invoke_shallow_step_x2

  !> TWO whole time steps of the GOcean leapfrog (update + Asselin filter of the old level, twice) in one launch (NE offset):
  !! level n+2 into unew2, vnew2, pnew2 and the filtered level n+1 into uold2, vold2, pold2; u .. pold are not modified.
  !! == two invoke_shallow_step_smooth calls with the usual rotation, bit for bit, at 48 instead of 96 B/cell/step.
  !! Time loop: ping-pong (u, v, p, uold, vold, pold) <-> (unew2, vnew2, pnew2, uold2, vold2, pold2).
  subroutine invoke_shallow_step_smooth_x2(prm, alpha, u, v, p, uold, vold, pold, unew2, vnew2, pnew2, uold2, vold2, pold2)
    type(c_sw_params), intent(in) :: prm
    real(go_wp), intent(in) :: alpha
    type(r2d_field), intent(inout), target :: u, v, p, uold, vold, pold, unew2, vnew2, pnew2, uold2, vold2, pold2
    integer(c_int) :: rc
    call need_device(u);  call need_device(v);  call need_device(p)
    call need_device(uold);  call need_device(vold);  call need_device(pold)
    call need_device(unew2);  call need_device(vnew2);  call need_device(pnew2)
    call need_device(uold2);  call need_device(vold2);  call need_device(pold2)
    rc = dlesm_shallow_step_smooth_x2_f64(prm, alpha, int(p%grid%nx, c_int), int(p%grid%ny, c_int), &
                                          int(p%internal%xstart, c_int), int(p%internal%xstop, c_int), &
                                          int(p%internal%ystart, c_int), int(p%internal%ystop, c_int), &
                                          field_device_data(u), field_device_data(v), field_device_data(p), &
                                          field_device_data(uold), field_device_data(vold), field_device_data(pold), &
                                          field_device_data(unew2), field_device_data(vnew2), field_device_data(pnew2), &
                                          field_device_data(uold2), field_device_data(vold2), field_device_data(pold2), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_shallow_step_smooth_x2: ' // dlesm_error_text())
  end subroutine invoke_shallow_step_smooth_x2

  !> Two steps of the SW-offset periodic model in one launch (== two invoke_shallow_step_sw_periodic calls): level n+1 with its
  !! periodic images into unew .. pnew, level n+2 with its images into unew2 .. pnew2.
  subroutine invoke_shallow_step_sw_x2_periodic(prm, u, v, p, uold, vold, pold, unew, vnew, pnew, unew2, vnew2, pnew2)
    type(c_sw_params), intent(in) :: prm
    type(r2d_field), intent(inout), target :: u, v, p, uold, vold, pold, unew, vnew, pnew, unew2, vnew2, pnew2
    type(c_region) :: cint
    integer(c_int) :: rc
    call need_device(u);  call need_device(v);  call need_device(p)
    call need_device(uold);  call need_device(vold);  call need_device(pold)
    call need_device(unew);  call need_device(vnew);  call need_device(pnew)
    call need_device(unew2);  call need_device(vnew2);  call need_device(pnew2)
    associate (it => p%internal)
      cint = c_region(it%nx, it%ny, it%xstart, it%xstop, it%ystart, it%ystop)
    end associate
    rc = dlesm_shallow_step_sw_x2_periodic_f64(prm, int(p%grid%nx, c_int), int(p%grid%ny, c_int), cint, &
                                               int(p%grid%boundary_conditions(1), c_int), int(p%grid%boundary_conditions(2), c_int), &
                                               field_device_data(u), field_device_data(v), field_device_data(p), &
                                               field_device_data(uold), field_device_data(vold), field_device_data(pold), &
                                               field_device_data(unew), field_device_data(vnew), field_device_data(pnew), &
                                               field_device_data(unew2), field_device_data(vnew2), field_device_data(pnew2), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_shallow_step_sw_x2_periodic: ' // dlesm_error_text())
  end subroutine invoke_shallow_step_sw_x2_periodic

  !> TWO whole time steps of the GOcean `shallow` benchmark in one launch: update, Asselin filter of the old level and periodic
  !! images, twice.  Level n+2 into unew2 .. pnew2, the filtered level n+1 into uold2 .. pold2 (both with their images); u .. pold
  !! are not modified.  == two invoke_shallow_step_sw_smooth_periodic calls with the loop's rotation, at 48 instead of 96 B/cell/step.
  subroutine invoke_shallow_step_sw_smooth_x2_periodic(prm, alpha, u, v, p, uold, vold, pold, unew2, vnew2, pnew2, uold2, vold2, pold2)
    type(c_sw_params), intent(in) :: prm
    real(go_wp), intent(in) :: alpha
    type(r2d_field), intent(inout), target :: u, v, p, uold, vold, pold, unew2, vnew2, pnew2, uold2, vold2, pold2
    type(c_region) :: cint
    integer(c_int) :: rc
    call need_device(u);  call need_device(v);  call need_device(p)
    call need_device(uold);  call need_device(vold);  call need_device(pold)
    call need_device(unew2);  call need_device(vnew2);  call need_device(pnew2)
    call need_device(uold2);  call need_device(vold2);  call need_device(pold2)
    associate (it => p%internal)
      cint = c_region(it%nx, it%ny, it%xstart, it%xstop, it%ystart, it%ystop)
    end associate
    rc = dlesm_shallow_step_sw_smooth_x2_periodic_f64(prm, alpha, int(p%grid%nx, c_int), int(p%grid%ny, c_int), cint, &
                                                      int(p%grid%boundary_conditions(1), c_int), &
                                                      int(p%grid%boundary_conditions(2), c_int), &
                                                      field_device_data(u), field_device_data(v), field_device_data(p), &
                                                      field_device_data(uold), field_device_data(vold), field_device_data(pold), &
                                                      field_device_data(unew2), field_device_data(vnew2), field_device_data(pnew2), &
                                                      field_device_data(uold2), field_device_data(vold2), field_device_data(pold2), &
                                                      c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_shallow_step_sw_smooth_x2_periodic: ' // dlesm_error_text())
  end subroutine invoke_shallow_step_sw_smooth_x2_periodic

  !> The same for the SW-offset periodic model: update, filter and the periodic images of the new and of the filtered old
  !! level in ONE launch -- a whole time step of the GOcean `shallow` benchmark.
  subroutine invoke_shallow_step_sw_smooth_periodic(prm, alpha, u, v, p, uold, vold, pold, unew, vnew, pnew)
    type(c_sw_params), intent(in) :: prm
    real(go_wp), intent(in) :: alpha
    type(r2d_field), intent(inout), target :: u, v, p, uold, vold, pold, unew, vnew, pnew
    type(c_region) :: cint
    integer(c_int) :: rc
    call need_device(u);  call need_device(v);  call need_device(p)
    call need_device(uold);  call need_device(vold);  call need_device(pold)
    call need_device(unew);  call need_device(vnew);  call need_device(pnew)
    associate (it => p%internal)
      cint = c_region(it%nx, it%ny, it%xstart, it%xstop, it%ystart, it%ystop)
    end associate
    rc = dlesm_shallow_step_sw_smooth_periodic_f64(prm, alpha, int(p%grid%nx, c_int), int(p%grid%ny, c_int), cint, &
                                                   int(p%grid%boundary_conditions(1), c_int), &
                                                   int(p%grid%boundary_conditions(2), c_int), &
                                                   field_device_data(u), field_device_data(v), field_device_data(p), &
                                                   field_device_data(uold), field_device_data(vold), field_device_data(pold), &
                                                   field_device_data(unew), field_device_data(vnew), field_device_data(pnew), &
                                                   c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_shallow_step_sw_smooth_periodic: ' // dlesm_error_text())
  end subroutine invoke_shallow_step_sw_smooth_periodic

  !> The distributed form of invoke_shallow_step_smooth (one launch + the exchange of the new level hidden behind the interior):
  !! `pipelined` = the time-loop form (halo_join(grid) after the loop); serial builds fall back to invoke_shallow_step_smooth.
  subroutine invoke_shallow_step_smooth_dm(prm, alpha, u, v, p, uold, vold, pold, unew, vnew, pnew, pipelined)
    use parallel_comms_mod, only: halo_plan_for, serial_plan_for
    use parallel_utils_mod, only: DIST_MEM_ENABLED
    type(c_sw_params), intent(in) :: prm
    real(go_wp), intent(in) :: alpha
    type(c_ptr) :: plan
    type(r2d_field), intent(inout), target :: u, v, p, uold, vold, pold, unew, vnew, pnew
    logical, intent(in), optional :: pipelined
    logical :: pipe
    integer(c_int) :: rc
    if (.not. DIST_MEM_ENABLED) then
       call invoke_shallow_step_smooth(prm, alpha, u, v, p, uold, vold, pold, unew, vnew, pnew)
       return
    end if
    pipe = .false.
    if (present(pipelined)) pipe = pipelined
    call need_device(u);  call need_device(v);  call need_device(p)
    call need_device(uold);  call need_device(vold);  call need_device(pold)
    call need_device(unew);  call need_device(vnew);  call need_device(pnew)
    if (pipe) then
       rc = dlesm_shallow_step_smooth_dm_pipelined(halo_plan_for(p%grid%nx, p%grid%ny), prm, alpha, &
                int(p%grid%nx, c_int), int(p%grid%ny, c_int), int(p%internal%xstart, c_int), int(p%internal%xstop, c_int), &
                int(p%internal%ystart, c_int), int(p%internal%ystop, c_int), &
                field_device_data(u), field_device_data(v), field_device_data(p), &
                field_device_data(uold), field_device_data(vold), field_device_data(pold), &
                field_device_data(unew), field_device_data(vnew), field_device_data(pnew), c_null_ptr)
    else
       rc = dlesm_shallow_step_smooth_dm(halo_plan_for(p%grid%nx, p%grid%ny), prm, alpha, &
                int(p%grid%nx, c_int), int(p%grid%ny, c_int), int(p%internal%xstart, c_int), int(p%internal%xstop, c_int), &
                int(p%internal%ystart, c_int), int(p%internal%ystop, c_int), &
                field_device_data(u), field_device_data(v), field_device_data(p), &
                field_device_data(uold), field_device_data(vold), field_device_data(pold), &
                field_device_data(unew), field_device_data(vnew), field_device_data(pnew), c_null_ptr)
    end if
    if (rc /= 0) call gocean_stop('invoke_shallow_step_smooth_dm: ' // dlesm_error_text())
  end subroutine invoke_shallow_step_smooth_dm

  !> plan_shallow_step for the SW-offset step
  subroutine plan_shallow_step_sw(prm, u, v, p, uold, vold, pold, unew, vnew, pnew)
    type(c_sw_params), intent(in) :: prm
    type(r2d_field), intent(inout), target :: u, v, p, uold, vold, pold, unew, vnew, pnew
    integer(c_int) :: rc
    call need_device(u);  call need_device(v);  call need_device(p)
    call need_device(uold);  call need_device(vold);  call need_device(pold)
    call need_device(unew);  call need_device(vnew);  call need_device(pnew)
    rc = dlesm_shallow_autotune_sw_f64(prm, int(p%grid%nx, c_int), int(p%grid%ny, c_int), &
                                       int(p%internal%xstart, c_int), int(p%internal%xstop, c_int), &
                                       int(p%internal%ystart, c_int), int(p%internal%ystop, c_int), &
                                       field_device_data(u), field_device_data(v), field_device_data(p), &
                                       field_device_data(uold), field_device_data(vold), field_device_data(pold), &
                                       field_device_data(unew), field_device_data(vnew), field_device_data(pnew), &
                                       c_null_ptr)
    if (rc /= 0) call gocean_stop('plan_shallow_step_sw: ' // dlesm_error_text())
  end subroutine plan_shallow_step_sw

  ! ---- The GOcean `shallow` kernels ONE BY ONE: what replaces each generated loop nest
  !        do jj = fld%internal%ystart, fld%internal%ystop
  !           do ji = fld%internal%xstart, fld%internal%xstop
  !              call compute_cu_code(ji, jj, cu%data, p%data, u%data)
  !      of an unmodified PSy layer (kernel form: reference infrastructure_mod.f90:13-41; metadata
  !      argument_mod.f90:39-112, kernel_mod.f90:28-50).  Loop bounds: the written field's internal region
  !      (ITERATES_OVER = GO_INTERNAL_PTS) unless `box` = (/xstart, xstop, ystart, ystop/) is given; the kernel's
  !      index_offset is the grid's; dx, dy (the kernels' GO_GRID_DX_CONST / GO_GRID_DY_CONST arguments) come from
  !      the grid.  Formulas: DESIGN.md sections 6, 6.2, 6.3.

  subroutine kernel_box(fld, box, b)
    type(r2d_field), intent(in) :: fld
    integer, intent(in), optional :: box(4)
    integer(c_int), intent(out) :: b(4)
    if (present(box)) then
       b = int(box, c_int)
    else
       b = int((/ fld%internal%xstart, fld%internal%xstop, fld%internal%ystart, fld%internal%ystop /), c_int)
    end if
  end subroutine kernel_box

  subroutine invoke_compute_cu(cu, p, u, box)
    type(r2d_field), intent(inout), target :: cu, p, u
    integer, intent(in), optional :: box(4)
    integer(c_int) :: rc, b(4)
    call need_device(cu);  call need_device(p);  call need_device(u)
    call kernel_box(cu, box, b)
    rc = dlesm_compute_cu_f64(int(cu%grid%offset, c_int), int(cu%grid%nx, c_int), int(cu%grid%ny, c_int), &
                              b(1), b(2), b(3), b(4), field_device_data(cu), field_device_data(p), &
                              field_device_data(u), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_compute_cu: ' // dlesm_error_text())
  end subroutine invoke_compute_cu

  subroutine invoke_compute_cv(cv, p, v, box)
    type(r2d_field), intent(inout), target :: cv, p, v
    integer, intent(in), optional :: box(4)
    integer(c_int) :: rc, b(4)
    call need_device(cv);  call need_device(p);  call need_device(v)
    call kernel_box(cv, box, b)
    rc = dlesm_compute_cv_f64(int(cv%grid%offset, c_int), int(cv%grid%nx, c_int), int(cv%grid%ny, c_int), &
                              b(1), b(2), b(3), b(4), field_device_data(cv), field_device_data(p), &
                              field_device_data(v), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_compute_cv: ' // dlesm_error_text())
  end subroutine invoke_compute_cv

  subroutine invoke_compute_z(z, p, u, v, box)
    type(r2d_field), intent(inout), target :: z, p, u, v
    integer, intent(in), optional :: box(4)
    integer(c_int) :: rc, b(4)
    call need_device(z);  call need_device(p);  call need_device(u);  call need_device(v)
    call kernel_box(z, box, b)
    rc = dlesm_compute_z_f64(int(z%grid%offset, c_int), int(z%grid%nx, c_int), int(z%grid%ny, c_int), &
                             b(1), b(2), b(3), b(4), 4.0_go_wp / z%grid%dx, 4.0_go_wp / z%grid%dy, &
                             field_device_data(z), field_device_data(p), field_device_data(u), field_device_data(v), &
                             c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_compute_z: ' // dlesm_error_text())
  end subroutine invoke_compute_z

  subroutine invoke_compute_h(h, p, u, v, box)
    type(r2d_field), intent(inout), target :: h, p, u, v
    integer, intent(in), optional :: box(4)
    integer(c_int) :: rc, b(4)
    call need_device(h);  call need_device(p);  call need_device(u);  call need_device(v)
    call kernel_box(h, box, b)
    rc = dlesm_compute_h_f64(int(h%grid%offset, c_int), int(h%grid%nx, c_int), int(h%grid%ny, c_int), &
                             b(1), b(2), b(3), b(4), field_device_data(h), field_device_data(p), &
                             field_device_data(u), field_device_data(v), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_compute_h: ' // dlesm_error_text())
  end subroutine invoke_compute_h

  !> tdt = 2*dt in a leapfrog step (dt in the first, forward step)
  subroutine invoke_compute_unew(unew, uold, z, cv, h, tdt, box)
    type(r2d_field), intent(inout), target :: unew, uold, z, cv, h
    real(go_wp), intent(in) :: tdt
    integer, intent(in), optional :: box(4)
    integer(c_int) :: rc, b(4)
    call need_device(unew);  call need_device(uold);  call need_device(z);  call need_device(cv);  call need_device(h)
    call kernel_box(unew, box, b)
    rc = dlesm_compute_unew_f64(int(unew%grid%offset, c_int), int(unew%grid%nx, c_int), int(unew%grid%ny, c_int), &
                                b(1), b(2), b(3), b(4), tdt / 8.0_go_wp, tdt / unew%grid%dx, &
                                field_device_data(unew), field_device_data(uold), field_device_data(z), &
                                field_device_data(cv), field_device_data(h), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_compute_unew: ' // dlesm_error_text())
  end subroutine invoke_compute_unew

  subroutine invoke_compute_vnew(vnew, vold, z, cu, h, tdt, box)
    type(r2d_field), intent(inout), target :: vnew, vold, z, cu, h
    real(go_wp), intent(in) :: tdt
    integer, intent(in), optional :: box(4)
    integer(c_int) :: rc, b(4)
    call need_device(vnew);  call need_device(vold);  call need_device(z);  call need_device(cu);  call need_device(h)
    call kernel_box(vnew, box, b)
    rc = dlesm_compute_vnew_f64(int(vnew%grid%offset, c_int), int(vnew%grid%nx, c_int), int(vnew%grid%ny, c_int), &
                                b(1), b(2), b(3), b(4), tdt / 8.0_go_wp, tdt / vnew%grid%dy, &
                                field_device_data(vnew), field_device_data(vold), field_device_data(z), &
                                field_device_data(cu), field_device_data(h), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_compute_vnew: ' // dlesm_error_text())
  end subroutine invoke_compute_vnew

  subroutine invoke_compute_pnew(pnew, pold, cu, cv, tdt, box)
    type(r2d_field), intent(inout), target :: pnew, pold, cu, cv
    real(go_wp), intent(in) :: tdt
    integer, intent(in), optional :: box(4)
    integer(c_int) :: rc, b(4)
    call need_device(pnew);  call need_device(pold);  call need_device(cu);  call need_device(cv)
    call kernel_box(pnew, box, b)
    rc = dlesm_compute_pnew_f64(int(pnew%grid%offset, c_int), int(pnew%grid%nx, c_int), int(pnew%grid%ny, c_int), &
                                b(1), b(2), b(3), b(4), tdt / pnew%grid%dx, tdt / pnew%grid%dy, &
                                field_device_data(pnew), field_device_data(pold), field_device_data(cu), &
                                field_device_data(cv), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_compute_pnew: ' // dlesm_error_text())
  end subroutine invoke_compute_pnew

  !> time_smooth (the Asselin filter of the leapfrog scheme), over field_old%internal:
  !!   field_old = field + alpha*(field_new - 2*field + field_old)
  subroutine invoke_time_smooth(field, field_new, field_old, alpha, box)
    type(r2d_field), intent(inout), target :: field, field_new, field_old
    real(go_wp), intent(in) :: alpha
    integer, intent(in), optional :: box(4)
    integer(c_int) :: rc, b(4)
    call need_device(field);  call need_device(field_new);  call need_device(field_old)
    call kernel_box(field_old, box, b)
    rc = dlesm_time_smooth_f64(int(field_old%grid%nx, c_int), int(field_old%grid%ny, c_int), b(1), b(2), b(3), b(4), &
                               alpha, field_device_data(field), field_device_data(field_new), &
                               field_device_data(field_old), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_time_smooth: ' // dlesm_error_text())
  end subroutine invoke_time_smooth

  !> The periodic-boundary copies of a field -- its halo(:) list (field_mod.f90:1394-1464), in order --
  !! on the device: what a periodic model's PSy layer does after every kernel that writes the field.
  subroutine invoke_periodic_halos(fld)
    type(r2d_field), intent(inout), target :: fld
    type(c_region) :: cint
    integer(c_int) :: rc
    if (fld%num_halos == 0) return
    call need_device(fld)
    associate (it => fld%internal)
      cint = c_region(it%nx, it%ny, it%xstart, it%xstop, it%ystart, it%ystop)
    end associate
    rc = dlesm_periodic_halos_apply_f64(field_device_data(fld), int(fld%grid%nx, c_int), int(fld%grid%ny, c_int), &
                                        cint, int(fld%grid%boundary_conditions(1), c_int), &
                                        int(fld%grid%boundary_conditions(2), c_int), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_periodic_halos: ' // dlesm_error_text())
  end subroutine invoke_periodic_halos

  !> invoke_periodic_halos of up to four fields of one grid and internal region in TWO launches (all x copies, then all y
  !! copies) instead of two per field: what follows compute_cu / cv / z / h, or the three kernels of the new time level
  subroutine invoke_periodic_halos_multi(f1, f2, f3, f4)
    type(r2d_field), intent(inout), target :: f1, f2
    type(r2d_field), intent(inout), target, optional :: f3, f4
    type(c_ptr) :: ptrs(4)
    type(c_region) :: cint
    integer(c_int) :: rc, n
    if (f1%num_halos == 0) return
    call need_device(f1);  call need_device(f2)
    ptrs(1) = field_device_data(f1);  ptrs(2) = field_device_data(f2);  n = 2
    if (present(f3)) then
       call need_device(f3);  n = n + 1;  ptrs(n) = field_device_data(f3)
    end if
    if (present(f4)) then
       call need_device(f4);  n = n + 1;  ptrs(n) = field_device_data(f4)
    end if
    associate (it => f1%internal)
      cint = c_region(it%nx, it%ny, it%xstart, it%xstop, it%ystart, it%ystop)
    end associate
    rc = dlesm_periodic_halos_apply_multi_f64(ptrs, n, int(f1%grid%nx, c_int), int(f1%grid%ny, c_int), cint, &
                                              int(f1%grid%boundary_conditions(1), c_int), &
                                              int(f1%grid%boundary_conditions(2), c_int), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_periodic_halos_multi: ' // dlesm_error_text())
  end subroutine invoke_periodic_halos_multi

  !> Optional planning call for invoke_shallow_step (like plan_jacobi5): the library times its
  !! launch shapes and cache policies on these fields once -- every trial is the same valid step
  !! into unew, vnew, pnew -- and keeps the fastest for this field geometry.
  subroutine plan_shallow_step(prm, u, v, p, uold, vold, pold, unew, vnew, pnew)
    type(c_sw_params), intent(in) :: prm
    type(r2d_field), intent(inout), target :: u, v, p, uold, vold, pold, unew, vnew, pnew
    integer(c_int) :: rc
    call need_device(u);  call need_device(v);  call need_device(p)
    call need_device(uold);  call need_device(vold);  call need_device(pold)
    call need_device(unew);  call need_device(vnew);  call need_device(pnew)
    rc = dlesm_shallow_autotune_f64(prm, int(p%grid%nx, c_int), int(p%grid%ny, c_int), &
                                    int(p%internal%xstart, c_int), int(p%internal%xstop, c_int), &
                                    int(p%internal%ystart, c_int), int(p%internal%ystop, c_int), &
                                    field_device_data(u), field_device_data(v), field_device_data(p), &
                                    field_device_data(uold), field_device_data(vold), field_device_data(pold), &
                                    field_device_data(unew), field_device_data(vnew), field_device_data(pnew), &
                                    c_null_ptr)
    if (rc /= 0) call gocean_stop('plan_shallow_step: ' // dlesm_error_text())
  end subroutine plan_shallow_step

  !> Distributed shallow-water step: u, v, p must have valid halos; unew, vnew, pnew leave with
  !! theirs, exchanged in ONE grouped RCCL launch that runs behind the interior sweep.
  subroutine invoke_shallow_step_dm(prm, u, v, p, uold, vold, pold, unew, vnew, pnew)
    use parallel_comms_mod, only: halo_plan_for
    use parallel_utils_mod, only: DIST_MEM_ENABLED
    type(c_sw_params), intent(in) :: prm
    type(r2d_field), intent(inout), target :: u, v, p, uold, vold, pold, unew, vnew, pnew
    integer(c_int) :: rc
    if (.not. DIST_MEM_ENABLED) then
       call invoke_shallow_step(prm, u, v, p, uold, vold, pold, unew, vnew, pnew)
       return
    end if
    call need_device(u);  call need_device(v);  call need_device(p)
    call need_device(uold);  call need_device(vold);  call need_device(pold)
    call need_device(unew);  call need_device(vnew);  call need_device(pnew)
    rc = dlesm_shallow_step_dm(halo_plan_for(p%grid%nx, p%grid%ny), prm, &
                               int(p%grid%nx, c_int), int(p%grid%ny, c_int), &
                               int(p%internal%xstart, c_int), int(p%internal%xstop, c_int), &
                               int(p%internal%ystart, c_int), int(p%internal%ystop, c_int), &
                               field_device_data(u), field_device_data(v), field_device_data(p), &
                               field_device_data(uold), field_device_data(vold), field_device_data(pold), &
                               field_device_data(unew), field_device_data(vnew), field_device_data(pnew), &
                               c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_shallow_step_dm: ' // dlesm_error_text())
  end subroutine invoke_shallow_step_dm

  !> TWO leapfrog steps and ONE depth-2 exchange on a decomposed grid (dlesm_shallow_step_x2_dm): the grid must have been
  !! decomposed with halo_width = 2 (without distributed memory the plan has no messages: the library runs the single-domain entry).  u, v, p need valid depth-2 halos, uold, vold, pold depth-1 halos; unew2, vnew2, pnew2 leave
  !! with valid depth-2 halos, unew, vnew, pnew valid on the internal region grown by one cell towards every neighbour.
  !! Time loop: (cur, old, new1, new2) <- (new2, new1, old, cur) after every call.
  subroutine invoke_shallow_step_x2_dm(prm, u, v, p, uold, vold, pold, unew, vnew, pnew, unew2, vnew2, pnew2)
    use parallel_comms_mod, only: halo_plan_for, serial_plan_for
    use parallel_utils_mod, only: DIST_MEM_ENABLED
    type(c_sw_params), intent(in) :: prm
    type(r2d_field), intent(inout), target :: u, v, p, uold, vold, pold, unew, vnew, pnew, unew2, vnew2, pnew2
    type(c_ptr) :: plan
    integer(c_int) :: rc
    if (p%grid%subdomain%internal%xstart - 1 /= 2 .or. p%grid%subdomain%internal%ystart - 1 /= 2) &
         call gocean_stop('invoke_shallow_step_x2_dm: the grid must be decomposed with halo_width = 2')
    call need_device(u);  call need_device(v);  call need_device(p)
    call need_device(uold);  call need_device(vold);  call need_device(pold)
    call need_device(unew);  call need_device(vnew);  call need_device(pnew)
    call need_device(unew2);  call need_device(vnew2);  call need_device(pnew2)
    if (DIST_MEM_ENABLED) then
       plan = halo_plan_for(p%grid%nx, p%grid%ny)
    else
       plan = serial_plan_for(p%grid%nx, p%grid%ny)
    end if
    rc = dlesm_shallow_step_x2_dm(plan, prm, int(p%grid%nx, c_int), int(p%grid%ny, c_int), &
                                  int(p%internal%xstart, c_int), int(p%internal%xstop, c_int), &
                                  int(p%internal%ystart, c_int), int(p%internal%ystop, c_int), &
                                  field_device_data(u), field_device_data(v), field_device_data(p), &
                                  field_device_data(uold), field_device_data(vold), field_device_data(pold), &
                                  field_device_data(unew), field_device_data(vnew), field_device_data(pnew), &
                                  field_device_data(unew2), field_device_data(vnew2), field_device_data(pnew2), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_shallow_step_x2_dm: ' // dlesm_error_text())
  end subroutine invoke_shallow_step_x2_dm

  !> TWO filtered leapfrog steps and ONE depth-2 exchange on a decomposed grid (dlesm_shallow_step_smooth_x2_dm; halo_width = 2):
  !! level n+2 into unew2, vnew2, pnew2 and the filtered level n+1 into uold2, vold2, pold2, both with valid depth-2 halos;
  !! u .. pold are not modified (the filtered old level needs valid depth-1 halos).
  !! Time loop: ping-pong (u, v, p, uold, vold, pold) <-> (unew2, vnew2, pnew2, uold2, vold2, pold2).
  subroutine invoke_shallow_step_smooth_x2_dm(prm, alpha, u, v, p, uold, vold, pold, unew2, vnew2, pnew2, uold2, vold2, pold2)
    use parallel_comms_mod, only: halo_plan_for, serial_plan_for
    use parallel_utils_mod, only: DIST_MEM_ENABLED
    type(c_sw_params), intent(in) :: prm
    real(go_wp), intent(in) :: alpha
    type(r2d_field), intent(inout), target :: u, v, p, uold, vold, pold, unew2, vnew2, pnew2, uold2, vold2, pold2
    type(c_ptr) :: plan
    integer(c_int) :: rc
    if (p%grid%subdomain%internal%xstart - 1 /= 2 .or. p%grid%subdomain%internal%ystart - 1 /= 2) &
         call gocean_stop('invoke_shallow_step_smooth_x2_dm: the grid must be decomposed with halo_width = 2')
    call need_device(u);  call need_device(v);  call need_device(p)
    call need_device(uold);  call need_device(vold);  call need_device(pold)
    call need_device(unew2);  call need_device(vnew2);  call need_device(pnew2)
    call need_device(uold2);  call need_device(vold2);  call need_device(pold2)
    if (DIST_MEM_ENABLED) then
       plan = halo_plan_for(p%grid%nx, p%grid%ny)
    else
       plan = serial_plan_for(p%grid%nx, p%grid%ny)
    end if
    rc = dlesm_shallow_step_smooth_x2_dm(plan, prm, alpha, &
                                         int(p%grid%nx, c_int), int(p%grid%ny, c_int), &
                                         int(p%internal%xstart, c_int), int(p%internal%xstop, c_int), &
                                         int(p%internal%ystart, c_int), int(p%internal%ystop, c_int), &
                                         field_device_data(u), field_device_data(v), field_device_data(p), &
                                         field_device_data(uold), field_device_data(vold), field_device_data(pold), &
                                         field_device_data(unew2), field_device_data(vnew2), field_device_data(pnew2), &
                                         field_device_data(uold2), field_device_data(vold2), field_device_data(pold2), c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_shallow_step_smooth_x2_dm: ' // dlesm_error_text())
  end subroutine invoke_shallow_step_smooth_x2_dm

  !> The same step for a time loop: returns with the exchange of the new fields in flight; the next
  !! invoke_shallow_step_dm_pipelined on this grid waits for it on the device; halo_join(grid) after the loop.
  subroutine invoke_shallow_step_dm_pipelined(prm, u, v, p, uold, vold, pold, unew, vnew, pnew)
    use parallel_comms_mod, only: halo_plan_for
    use parallel_utils_mod, only: DIST_MEM_ENABLED
    type(c_sw_params), intent(in) :: prm
    type(r2d_field), intent(inout), target :: u, v, p, uold, vold, pold, unew, vnew, pnew
    integer(c_int) :: rc
    if (.not. DIST_MEM_ENABLED) then
       call invoke_shallow_step(prm, u, v, p, uold, vold, pold, unew, vnew, pnew)
       return
    end if
    call need_device(u);  call need_device(v);  call need_device(p)
    call need_device(uold);  call need_device(vold);  call need_device(pold)
    call need_device(unew);  call need_device(vnew);  call need_device(pnew)
    rc = dlesm_shallow_step_dm_pipelined(halo_plan_for(p%grid%nx, p%grid%ny), prm, &
                               int(p%grid%nx, c_int), int(p%grid%ny, c_int), &
                               int(p%internal%xstart, c_int), int(p%internal%xstop, c_int), &
                               int(p%internal%ystart, c_int), int(p%internal%ystop, c_int), &
                               field_device_data(u), field_device_data(v), field_device_data(p), &
                               field_device_data(uold), field_device_data(vold), field_device_data(pold), &
                               field_device_data(unew), field_device_data(vnew), field_device_data(pnew), &
                               c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_shallow_step_dm_pipelined: ' // dlesm_error_text())
  end subroutine invoke_shallow_step_dm_pipelined

  !> halo_exchange(1) of several fields of one grid in a single grouped RCCL launch
  subroutine halo_exchange_multi(f1, f2, f3)
    use parallel_comms_mod, only: halo_plan_for
    use parallel_utils_mod, only: DIST_MEM_ENABLED
    type(r2d_field), intent(inout), target :: f1, f2
    type(r2d_field), intent(inout), target, optional :: f3
    type(c_ptr) :: ptrs(3)
    integer(c_int) :: rc, n
    if (.not. DIST_MEM_ENABLED) return
    call need_device(f1);  call need_device(f2)
    ptrs(1) = field_device_data(f1);  ptrs(2) = field_device_data(f2);  n = 2
    if (present(f3)) then
       call need_device(f3)
       ptrs(3) = field_device_data(f3);  n = 3
    end if
    rc = dlesm_halo_exchange_multi_f64(halo_plan_for(f1%grid%nx, f1%grid%ny), ptrs, n, DLESM_DIRS_ALL, c_null_ptr)
    if (rc /= 0) call gocean_stop('halo_exchange_multi: ' // dlesm_error_text())
  end subroutine halo_exchange_multi

  !> Device mirrors of the grid properties a kernel may request through its metadata
  !! (GO_GRID_MASK_T, GO_GRID_DX_T, GO_GRID_AREA_T, ... argument_mod): fills the `*_device`
  !! pointers of grid_type (reference grid_mod.f90:104-150) with HBM copies of the host arrays.
  !! Idempotent; arrays keep the field layout (grid%nx x grid%ny, column-major).
  subroutine grid_to_device(grid)
    type(grid_type), intent(inout), target :: grid
    integer(c_size_t) :: nb
    nb = int(grid%nx, c_size_t) * int(grid%ny, c_size_t) * 8_c_size_t
    if (.not. c_associated(grid%tmask_device) .and. allocated(grid%tmask)) then
       if (hipMalloc(grid%tmask_device, nb / 2) /= 0) call gocean_stop('grid_to_device: hipMalloc failed')
       if (hipMemcpy(grid%tmask_device, c_loc(grid%tmask), nb / 2, 1_c_int) /= 0) &
            call gocean_stop('grid_to_device: upload failed')
    end if
    call mirror(grid%dx_t, grid%dx_t_device);  call mirror(grid%dy_t, grid%dy_t_device)
    call mirror(grid%dx_u, grid%dx_u_device);  call mirror(grid%dy_u, grid%dy_u_device)
    call mirror(grid%dx_v, grid%dx_v_device);  call mirror(grid%dy_v, grid%dy_v_device)
    call mirror(grid%dx_f, grid%dx_f_device);  call mirror(grid%dy_f, grid%dy_f_device)
    call mirror(grid%area_t, grid%area_t_device);  call mirror(grid%area_u, grid%area_u_device)
    call mirror(grid%area_v, grid%area_v_device)
    call mirror(grid%gphiu, grid%gphiu_device);  call mirror(grid%gphiv, grid%gphiv_device)
    call mirror(grid%gphif, grid%gphif_device)
    call mirror(grid%xt, grid%xt_device);  call mirror(grid%yt, grid%yt_device)
  contains
    subroutine mirror(host, dev)
      real(go_wp), allocatable, target, intent(in) :: host(:,:)
      type(c_ptr), intent(inout) :: dev
      if (c_associated(dev) .or. .not. allocated(host)) return
      if (hipMalloc(dev, nb) /= 0) call gocean_stop('grid_to_device: hipMalloc failed')
      if (hipMemcpy(dev, c_loc(host), nb, 1_c_int) /= 0) call gocean_stop('grid_to_device: upload failed')
    end subroutine mirror
  end subroutine grid_to_device

  !> The `copy` kernel of infrastructure_mod over all points
  subroutine invoke_copy(out, in)
    type(r2d_field), intent(inout), target :: out, in
    call need_device(in);  call need_device(out)
    call copy_field(in, out)
  end subroutine invoke_copy

  !> Synthetic initial condition: a hash of the GLOBAL cell index on the field's whole region
  subroutine invoke_hash_init(fld, seed, internal_only)
    type(r2d_field), intent(inout), target :: fld
    integer(c_int64_t), intent(in) :: seed
    logical, intent(in), optional :: internal_only    !< fill the internal region only (default: whole)
    integer(c_int) :: rc
    integer :: bx0, bx1, by0, by1
    integer(c_int64_t) :: gx0, gy0
    call need_device(fld)
    gx0 = fld%grid%subdomain%global%xstart - fld%grid%subdomain%internal%xstart + 1
    gy0 = fld%grid%subdomain%global%ystart - fld%grid%subdomain%internal%ystart + 1
    bx0 = fld%whole%xstart;  bx1 = fld%whole%xstop;  by0 = fld%whole%ystart;  by1 = fld%whole%ystop
    if (present(internal_only)) then
       if (internal_only) then
          bx0 = fld%internal%xstart;  bx1 = fld%internal%xstop
          by0 = fld%internal%ystart;  by1 = fld%internal%ystop
       end if
    end if
    rc = dlesm_hash_init_f64(field_device_data(fld), int(fld%grid%nx, c_int), int(fld%grid%ny, c_int), &
                             int(bx0, c_int), int(bx1, c_int), int(by0, c_int), int(by1, c_int), seed, gx0, gy0, &
                             c_null_ptr)
    if (rc /= 0) call gocean_stop('invoke_hash_init: ' // dlesm_error_text())
  end subroutine invoke_hash_init

end module dlesm_psy_mod
