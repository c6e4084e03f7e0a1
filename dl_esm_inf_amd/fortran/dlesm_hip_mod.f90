!> ISO_C_BINDING view of include/dlesm_hip.h: the thin layer between the Fortran
!! API modules and libdlesm_hip.so.  One interface block per C entry point, the
!! interoperable mirrors of the C structs, and nothing else.
module dlesm_hip_mod
  use iso_c_binding
  implicit none
  public

  integer(c_int), parameter :: DLESM_OK = 0, DLESM_EINVAL = -1, DLESM_ENODEV = -2, &
       DLESM_EHIP = -3, DLESM_ERCCL = -4, DLESM_EABORT = -5, DLESM_ECOMMS = -12
  integer, parameter :: DLESM_MAXCOMM = 16
  integer, parameter :: DLESM_UNIQUE_ID_BYTES = 128
  !> dirs_mask values of dlesm_halo_exchange_f64 (include/dlesm_hip.h)
  integer(c_int), parameter :: DLESM_DIRS_ALL = 15_c_int, DLESM_DIRS_NO_DIAGONALS = 16_c_int
  integer, parameter :: DLESM_TRACER_MAX = 8           ! dlesm_tracer_step_f64
  ! the tracer scheme of dlesm_nemolite_coupled_step_dm (DESIGN.md section 6.13)
  integer(c_int), parameter :: DLESM_TRACER_UPWIND = 0_c_int, DLESM_TRACER_MUSCL = 1_c_int, DLESM_TRACER_HANCOCK = 2_c_int
  !> norm values of dlesm_stencil5_resid_f64
  integer(c_int), parameter :: DLESM_NORM_MAX = 0_c_int, DLESM_NORM_SUMSQ = 1_c_int
  !> `what` values of dlesm_field_locate_f64, and the most fields one dlesm_field_stats_f64 call takes
  integer(c_int), parameter :: DLESM_LOCATE_NONFINITE = 0_c_int, DLESM_LOCATE_EQUAL = 1_c_int
  integer(c_int), parameter :: DLESM_STATS_MAX_FIELDS = 8_c_int

  !> struct dlesm_region
  type, bind(C) :: c_region
     integer(c_int) :: nx, ny, xstart, xstop, ystart, ystop
  end type c_region

  !> struct dlesm_subdomain
  type, bind(C) :: c_subdomain
     type(c_region) :: global, internal
  end type c_subdomain

  !> struct dlesm_decomp
  type, bind(C) :: c_decomp
     integer(c_int) :: global_nx, global_ny, nx, ny, ndomains, max_width, max_height
  end type c_decomp

  !> struct dlesm_comm_tables
  type, bind(C) :: c_comm_tables
     integer(c_int) :: nsend, nrecv
     integer(c_int), dimension(DLESM_MAXCOMM) :: dirsend, destination, isrcsend, jsrcsend, &
          idessend, jdessend, nxsend, nysend, dirrecv, source, isrcrecv, jsrcrecv, &
          idesrecv, jdesrecv, nxrecv, nyrecv
  end type c_comm_tables

  !> struct dlesm_sw_params
  type, bind(C) :: c_sw_params
     real(c_double) :: fsdx, fsdy, tdts8, tdtsdx, tdtsdy
  end type c_sw_params

  !> struct dlesm_momentum_params (DESIGN.md section 6.5)
  type, bind(C) :: c_momentum_params
     real(c_double) :: rdt, cbfr, visc, g
  end type c_momentum_params

  !> struct dlesm_momentum_grid: device pointers of the grid properties the momentum kernels read
  type, bind(C) :: c_momentum_grid
     type(c_ptr) :: tmask, dx_t, dy_t, dx_u, dy_u, dx_v, dy_v, area_u, area_v, fcor_u, fcor_v
  end type c_momentum_grid

  !> struct dlesm_field_stats (DESIGN.md section 5.5): 48 bytes
  type, bind(C) :: field_stats_type
     real(c_double) :: min, max, sum, sumsq
     integer(c_int64_t) :: count, nonfinite
  end type field_stats_type

  !> struct dlesm_tracer_courant (DESIGN.md section 6.14): 64 bytes.  The indices are 0-based linear, (j-1)*ld + (i-1); -1: none
  type, bind(C) :: tracer_courant_type
     real(c_double) :: face_max, outflow_max
     integer(c_int64_t) :: face_index, outflow_index, face_over, outflow_over, invalid, wet
  end type tracer_courant_type

  !> struct dlesm_flow_courant (DESIGN.md section 6.15): 128 bytes.  The indices are 0-based linear, (j-1)*ld + (i-1); -1: none
  type, bind(C) :: flow_courant_type
     real(c_double) :: gravity_max, advective_max, viscous_max, depth_min
     integer(c_int64_t) :: gravity_index, advective_index, viscous_index, depth_index
     integer(c_int64_t) :: gravity_over, advective_over, viscous_over, shallow, invalid, wet
     integer(c_int64_t) :: reserved(2)
  end type flow_courant_type

  !> A set of drifters on the device (DESIGN.md section 6.17): the number of particles and the dlesm_drifters handle that
  !! owns their positions and statuses (dlesm_psy_mod: drifters_create, drifters_get, drifters_free, drifter_step,
  !! particle_sort, particle_origin, cell_bin)
  type :: drifters_type
     integer(c_long_long) :: n = 0
     type(c_ptr) :: handle = c_null_ptr
  end type drifters_type
  integer(c_int), parameter :: DLESM_DRIFTER_ACTIVE = 0, DLESM_DRIFTER_LEFT = 1, DLESM_DRIFTER_OPEN = 2, &
                               DLESM_DRIFTER_GROUNDED = 3, DLESM_DRIFTER_FREE = 4

  interface
     ! ---- host-side index maps -------------------------------------------
     function dlesm_alignment_from_env(alignment) bind(C, name="dlesm_alignment_from_env") result(rc)
       import :: c_int
       integer(c_int), intent(out) :: alignment
       integer(c_int) :: rc
     end function
     function dlesm_grid_extents(sub_nx, sub_ny, alignment, nx, ny) &
          bind(C, name="dlesm_grid_extents") result(rc)
       import :: c_int
       integer(c_int), value :: sub_nx, sub_ny, alignment
       integer(c_int), intent(out) :: nx, ny
       integer(c_int) :: rc
     end function
     function dlesm_field_bounds(grid_points, offset, bc_x, bc_y, sub_internal, grid_nx, &
          grid_ny, internal, whole) bind(C, name="dlesm_field_bounds") result(rc)
       import :: c_int, c_region
       integer(c_int), value :: grid_points, offset, bc_x, bc_y, grid_nx, grid_ny
       type(c_region), intent(in) :: sub_internal
       type(c_region), intent(out) :: internal, whole
       integer(c_int) :: rc
     end function
     function dlesm_decompose(domainx, domainy, ndomains, ntilex, ntiley, halo_width, &
          decomp, subdomains) bind(C, name="dlesm_decompose") result(rc)
       import :: c_int, c_decomp, c_subdomain
       integer(c_int), value :: domainx, domainy, ndomains, ntilex, ntiley, halo_width
       type(c_decomp), intent(out) :: decomp
       type(c_subdomain), intent(out) :: subdomains(*)
       integer(c_int) :: rc
     end function
     function dlesm_iprocmap(decomp, subdomains, nranks, ia, ja) &
          bind(C, name="dlesm_iprocmap") result(owner)
       import :: c_int, c_decomp, c_subdomain
       type(c_decomp), intent(in) :: decomp
       type(c_subdomain), intent(in) :: subdomains(*)
       integer(c_int), value :: nranks, ia, ja
       integer(c_int) :: owner
     end function
     function dlesm_map_comms_depth(decomp, subdomains, nranks, rank1, depth, tables) &
          bind(C, name="dlesm_map_comms_depth") result(rc)
       import :: c_int, c_decomp, c_subdomain, c_comm_tables
       type(c_decomp), intent(in) :: decomp
       type(c_subdomain), intent(in) :: subdomains(*)
       integer(c_int), value :: nranks, rank1, depth
       type(c_comm_tables), intent(out) :: tables
       integer(c_int) :: rc
     end function
     function dlesm_map_comms(decomp, subdomains, nranks, rank1, tables) &
          bind(C, name="dlesm_map_comms") result(rc)
       import :: c_int, c_decomp, c_subdomain, c_comm_tables
       type(c_decomp), intent(in) :: decomp
       type(c_subdomain), intent(in) :: subdomains(*)
       integer(c_int), value :: nranks, rank1
       type(c_comm_tables), intent(out) :: tables
       integer(c_int) :: rc
     end function
     ! ---- runtime ----------------------------------------------------------
     function dlesm_last_error() bind(C, name="dlesm_last_error") result(msg)
       import :: c_ptr
       type(c_ptr) :: msg
     end function
     function dlesm_device_count() bind(C, name="dlesm_device_count") result(n)
       import :: c_int
       integer(c_int) :: n
     end function
     function dlesm_init(device) bind(C, name="dlesm_init") result(rc)
       import :: c_int
       integer(c_int), value :: device
       integer(c_int) :: rc
     end function
     function dlesm_finalize() bind(C, name="dlesm_finalize") result(rc)
       import :: c_int
       integer(c_int) :: rc
     end function
     ! ---- device fields ----------------------------------------------------
     function dlesm_field_create(ld, ny, field) bind(C, name="dlesm_field_create") result(rc)
       import :: c_int, c_ptr
       integer(c_int), value :: ld, ny
       type(c_ptr), intent(out) :: field
       integer(c_int) :: rc
     end function
     function dlesm_field_destroy(field) bind(C, name="dlesm_field_destroy") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: field
       integer(c_int) :: rc
     end function
     function dlesm_field_data(field) bind(C, name="dlesm_field_data") result(p)
       import :: c_ptr
       type(c_ptr), value :: field
       type(c_ptr) :: p
     end function
     !> the two C-flavour callbacks of field_mod (reference field_mod.f90:65-73,86-94)
     subroutine dlesm_read_from_device(from, to, startx, starty, nx, ny, blocking) &
          bind(C, name="dlesm_read_from_device")
       import :: c_ptr, c_int, c_bool
       type(c_ptr), intent(in), value :: from, to
       integer(c_int), intent(in), value :: startx, starty, nx, ny
       logical(c_bool), intent(in), value :: blocking
     end subroutine
     subroutine dlesm_write_to_device(from, to, startx, starty, nx, ny, blocking) &
          bind(C, name="dlesm_write_to_device")
       import :: c_ptr, c_int, c_bool
       type(c_ptr), intent(in), value :: from, to
       integer(c_int), intent(in), value :: startx, starty, nx, ny
       logical(c_bool), intent(in), value :: blocking
     end subroutine
     function dlesm_transfer_sync() bind(C, name="dlesm_transfer_sync") result(rc)
       import :: c_int
       integer(c_int) :: rc
     end function
     ! ---- kernels ------------------------------------------------------------
     function dlesm_stencil5_f64(in, out, ld, ny, xstart, xstop, ystart, ystop, stream) &
          bind(C, name="dlesm_stencil5_f64") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: in, out, stream
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       integer(c_int) :: rc
     end function
     function dlesm_stencil5_resid_f64(in, out, ld, ny, xstart, xstop, ystart, ystop, norm, result_dev, stream) &
          bind(C, name="dlesm_stencil5_resid_f64") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: in, out, result_dev, stream
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop, norm
       integer(c_int) :: rc
     end function
     function dlesm_stencil9_f64(in, out, coef, ld, ny, xstart, xstop, ystart, ystop, stream) &
          bind(C, name="dlesm_stencil9_f64") result(rc)
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: in, out, stream
       real(c_double), intent(in) :: coef(9)
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       integer(c_int) :: rc
     end function
     function dlesm_stencil9_step_dm(plan, in, out, coef, ld, ny, xstart, xstop, ystart, ystop, stream) &
          bind(C, name="dlesm_stencil9_step_dm") result(rc)
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: plan, in, out, stream
       real(c_double), intent(in) :: coef(9)
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       integer(c_int) :: rc
     end function
     function dlesm_continuity_f64(rdt, ld, ny, xstart, xstop, ystart, ystop, sshn_t, sshn_u, sshn_v, hu, hv, &
          un, vn, area_t, ssha, stream) bind(C, name="dlesm_continuity_f64") result(rc)
       import :: c_int, c_ptr, c_double
       real(c_double), value :: rdt
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: sshn_t, sshn_u, sshn_v, hu, hv, un, vn, area_t, ssha, stream
       integer(c_int) :: rc
     end function
     ! ---- NEMOLite2D-class momentum and sea-surface-height interpolation (DESIGN.md section 6.5)
     function dlesm_momentum_u_f64(params, grid, ld, ny, xstart, xstop, ystart, ystop, un, vn, ht, sshn_t, hu, sshn_u, &
          hv, sshn_v, ssha_u, ua, stream) bind(C, name="dlesm_momentum_u_f64") result(rc)
       import :: c_int, c_ptr, c_momentum_params, c_momentum_grid
       type(c_momentum_params), intent(in) :: params
       type(c_momentum_grid), intent(in) :: grid
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, ua, stream
       integer(c_int) :: rc
     end function
     function dlesm_momentum_v_f64(params, grid, ld, ny, xstart, xstop, ystart, ystop, un, vn, ht, sshn_t, hu, sshn_u, &
          hv, sshn_v, ssha_v, va, stream) bind(C, name="dlesm_momentum_v_f64") result(rc)
       import :: c_int, c_ptr, c_momentum_params, c_momentum_grid
       type(c_momentum_params), intent(in) :: params
       type(c_momentum_grid), intent(in) :: grid
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_v, va, stream
       integer(c_int) :: rc
     end function
     function dlesm_momentum_f64(params, grid, ld, ny, ubox, vbox, un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, &
          ssha_u, ssha_v, ua, va, stream) bind(C, name="dlesm_momentum_f64") result(rc)
       import :: c_int, c_ptr, c_momentum_params, c_momentum_grid, c_region
       type(c_momentum_params), intent(in) :: params
       type(c_momentum_grid), intent(in) :: grid
       integer(c_int), value :: ld, ny
       type(c_region), intent(in) :: ubox, vbox
       type(c_ptr), value :: un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, ssha_v, ua, va, stream
       integer(c_int) :: rc
     end function
     function dlesm_next_sshu_f64(ld, ny, xstart, xstop, ystart, ystop, tmask, area_t, area_u, sshn_t, sshn_u, stream) &
          bind(C, name="dlesm_next_sshu_f64") result(rc)
       import :: c_int, c_ptr
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: tmask, area_t, area_u, sshn_t, sshn_u, stream
       integer(c_int) :: rc
     end function
     function dlesm_next_sshv_f64(ld, ny, xstart, xstop, ystart, ystop, tmask, area_t, area_v, sshn_t, sshn_v, stream) &
          bind(C, name="dlesm_next_sshv_f64") result(rc)
       import :: c_int, c_ptr
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: tmask, area_t, area_v, sshn_t, sshn_v, stream
       integer(c_int) :: rc
     end function
     ! ---- open boundary: bc_ssh and Flather (DESIGN.md section 6.6)
     function dlesm_obc_create(tmask_host, ld, ny, tbox, ubox, vbox, plan) bind(C, name="dlesm_obc_create") result(rc)
       import :: c_int, c_ptr, c_region
       type(c_ptr), value :: tmask_host
       integer(c_int), value :: ld, ny
       type(c_region), intent(in) :: tbox, ubox, vbox
       type(c_ptr), intent(out) :: plan
       integer(c_int) :: rc
     end function
     function dlesm_obc_destroy(plan) bind(C, name="dlesm_obc_destroy") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: plan
       integer(c_int) :: rc
     end function
     function dlesm_obc_counts(plan, nt, nu, nv) bind(C, name="dlesm_obc_counts") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: plan
       integer(c_int), intent(out) :: nt, nu, nv
       integer(c_int) :: rc
     end function
     function dlesm_bc_ssh_f64(plan, ssh_bc, ssha, stream) bind(C, name="dlesm_bc_ssh_f64") result(rc)
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: plan
       real(c_double), value :: ssh_bc
       type(c_ptr), value :: ssha, stream
       integer(c_int) :: rc
     end function
     function dlesm_bc_flather_u_f64(plan, params, hu, sshn_u, sshn_t, ua, stream) bind(C, name="dlesm_bc_flather_u_f64") &
          result(rc)
       import :: c_int, c_ptr, c_momentum_params
       type(c_ptr), value :: plan
       type(c_momentum_params), intent(in) :: params
       type(c_ptr), value :: hu, sshn_u, sshn_t, ua, stream
       integer(c_int) :: rc
     end function
     function dlesm_bc_flather_v_f64(plan, params, hv, sshn_v, sshn_t, va, stream) bind(C, name="dlesm_bc_flather_v_f64") &
          result(rc)
       import :: c_int, c_ptr, c_momentum_params
       type(c_ptr), value :: plan
       type(c_momentum_params), intent(in) :: params
       type(c_ptr), value :: hv, sshn_v, sshn_t, va, stream
       integer(c_int) :: rc
     end function
     function dlesm_bc_open_f64(plan, params, ssh_bc, hu, sshn_u, hv, sshn_v, sshn_t, ssha, ua, va, stream) &
          bind(C, name="dlesm_bc_open_f64") result(rc)
       import :: c_int, c_ptr, c_double, c_momentum_params
       type(c_ptr), value :: plan
       type(c_momentum_params), intent(in) :: params
       real(c_double), value :: ssh_bc
       type(c_ptr), value :: hu, sshn_u, hv, sshn_v, sshn_t, ssha, ua, va, stream
       integer(c_int) :: rc
     end function
     function dlesm_nemolite_step_f64(params, grid, area_t, ld, ny, tbox, ubox, vbox, obc, ssh_bc, un, vn, ht, hu, hv, &
          sshn_t, sshn_u, sshn_v, ssha, ssha_u, ssha_v, ua, va, stream) bind(C, name="dlesm_nemolite_step_f64") result(rc)
       import :: c_int, c_ptr, c_double, c_momentum_params, c_momentum_grid, c_region
       type(c_momentum_params), intent(in) :: params
       type(c_momentum_grid), intent(in) :: grid
       type(c_ptr), value :: area_t
       integer(c_int), value :: ld, ny
       type(c_region), intent(in) :: tbox, ubox, vbox
       type(c_ptr), value :: obc
       real(c_double), value :: ssh_bc
       type(c_ptr), value :: un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, ssha, ssha_u, ssha_v, ua, va, stream
       integer(c_int) :: rc
     end function
     ! ---- land: the wet plan and the step that takes one (DESIGN.md section 6.9)
     function dlesm_wet_plan_create(tmask_host, ld, ny, box, plan) bind(C, name="dlesm_wet_plan_create") result(rc)
       import :: c_int, c_ptr, c_region
       type(c_ptr), value :: tmask_host
       integer(c_int), value :: ld, ny
       type(c_region), intent(in) :: box
       type(c_ptr), intent(out) :: plan
       integer(c_int) :: rc
     end function
     function dlesm_wet_plan_destroy(plan) bind(C, name="dlesm_wet_plan_destroy") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: plan
       integer(c_int) :: rc
     end function
     function dlesm_wet_plan_counts(plan, tiles, active) bind(C, name="dlesm_wet_plan_counts") result(rc)
       import :: c_int, c_ptr, c_long_long
       type(c_ptr), value :: plan
       integer(c_long_long), intent(out) :: tiles, active
       integer(c_int) :: rc
     end function
     function dlesm_nemolite_step_wet_f64(wet, params, grid, area_t, ld, ny, tbox, ubox, vbox, obc, ssh_bc, un, vn, ht, hu, &
          hv, sshn_t, sshn_u, sshn_v, ssha, ssha_u, ssha_v, ua, va, stream) bind(C, name="dlesm_nemolite_step_wet_f64") &
          result(rc)
       import :: c_int, c_ptr, c_double, c_momentum_params, c_momentum_grid, c_region
       type(c_ptr), value :: wet
       type(c_momentum_params), intent(in) :: params
       type(c_momentum_grid), intent(in) :: grid
       type(c_ptr), value :: area_t
       integer(c_int), value :: ld, ny
       type(c_region), intent(in) :: tbox, ubox, vbox
       type(c_ptr), value :: obc
       real(c_double), value :: ssh_bc
       type(c_ptr), value :: un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, ssha, ssha_u, ssha_v, ua, va, stream
       integer(c_int) :: rc
     end function
     function dlesm_stencil5_masked_f64(in, out, tmask, ld, ny, xstart, xstop, ystart, ystop, stream) &
          bind(C, name="dlesm_stencil5_masked_f64") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: in, out, tmask, stream
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       integer(c_int) :: rc
     end function
     function dlesm_shallow_step_f64(params, ld, ny, xstart, xstop, ystart, ystop, u, v, p, &
          uold, vold, pold, unew, vnew, pnew, stream) bind(C, name="dlesm_shallow_step_f64") result(rc)
       import :: c_int, c_ptr, c_sw_params
       type(c_sw_params), intent(in) :: params
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: u, v, p, uold, vold, pold, unew, vnew, pnew, stream
       integer(c_int) :: rc
     end function
     function dlesm_shallow_step_sw_f64(params, ld, ny, xstart, xstop, ystart, ystop, u, v, p, &
          uold, vold, pold, unew, vnew, pnew, stream) bind(C, name="dlesm_shallow_step_sw_f64") result(rc)
       import :: c_int, c_ptr, c_sw_params
       type(c_sw_params), intent(in) :: params
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: u, v, p, uold, vold, pold, unew, vnew, pnew, stream
       integer(c_int) :: rc
     end function
     function dlesm_shallow_step_sw_periodic_f64(params, ld, ny, internal, bc_x, bc_y, u, v, p, &
          uold, vold, pold, unew, vnew, pnew, stream) bind(C, name="dlesm_shallow_step_sw_periodic_f64") result(rc)
       import :: c_int, c_ptr, c_sw_params, c_region
       type(c_sw_params), intent(in) :: params
       integer(c_int), value :: ld, ny, bc_x, bc_y
       type(c_region), intent(in) :: internal
       type(c_ptr), value :: u, v, p, uold, vold, pold, unew, vnew, pnew, stream
       integer(c_int) :: rc
     end function
     function dlesm_shallow_step_x2_f64(params, ld, ny, xstart, xstop, ystart, ystop, u, v, p, uold, vold, pold, &
          unew, vnew, pnew, unew2, vnew2, pnew2, stream) bind(C, name="dlesm_shallow_step_x2_f64") result(rc)
       import :: c_int, c_ptr, c_sw_params
       type(c_sw_params), intent(in) :: params
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: u, v, p, uold, vold, pold, unew, vnew, pnew, unew2, vnew2, pnew2, stream
       integer(c_int) :: rc
     end function
     function dlesm_shallow_step_sw_x2_periodic_f64(params, ld, ny, internal, bc_x, bc_y, u, v, p, uold, vold, pold, &
          unew, vnew, pnew, unew2, vnew2, pnew2, stream) bind(C, name="dlesm_shallow_step_sw_x2_periodic_f64") result(rc)
       import :: c_int, c_ptr, c_sw_params, c_region
       type(c_sw_params), intent(in) :: params
       integer(c_int), value :: ld, ny, bc_x, bc_y
       type(c_region), intent(in) :: internal
       type(c_ptr), value :: u, v, p, uold, vold, pold, unew, vnew, pnew, unew2, vnew2, pnew2, stream
       integer(c_int) :: rc
     end function
     function dlesm_shallow_step_sw_smooth_x2_periodic_f64(params, alpha, ld, ny, internal, bc_x, bc_y, u, v, p, uold, vold, pold, &
          unew2, vnew2, pnew2, uold2, vold2, pold2, stream) bind(C, name="dlesm_shallow_step_sw_smooth_x2_periodic_f64") result(rc)
       import :: c_int, c_ptr, c_sw_params, c_region, c_double
       type(c_sw_params), intent(in) :: params
       real(c_double), value :: alpha
       integer(c_int), value :: ld, ny, bc_x, bc_y
       type(c_region), intent(in) :: internal
       type(c_ptr), value :: u, v, p, uold, vold, pold, unew2, vnew2, pnew2, uold2, vold2, pold2, stream
       integer(c_int) :: rc
     end function
     function dlesm_shallow_step_smooth_x2_f64(params, alpha, ld, ny, xstart, xstop, ystart, ystop, u, v, p, uold, vold, pold, &
          unew2, vnew2, pnew2, uold2, vold2, pold2, stream) bind(C, name="dlesm_shallow_step_smooth_x2_f64") result(rc)
       import :: c_int, c_ptr, c_sw_params, c_double
       type(c_sw_params), intent(in) :: params
       real(c_double), value :: alpha
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: u, v, p, uold, vold, pold, unew2, vnew2, pnew2, uold2, vold2, pold2, stream
       integer(c_int) :: rc
     end function
     function dlesm_shallow_step_smooth_f64(params, alpha, ld, ny, xstart, xstop, ystart, ystop, u, v, p, &
          uold, vold, pold, unew, vnew, pnew, stream) bind(C, name="dlesm_shallow_step_smooth_f64") result(rc)
       import :: c_int, c_ptr, c_sw_params, c_double
       type(c_sw_params), intent(in) :: params
       real(c_double), value :: alpha
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: u, v, p, uold, vold, pold, unew, vnew, pnew, stream
       integer(c_int) :: rc
     end function
     function dlesm_shallow_step_sw_smooth_periodic_f64(params, alpha, ld, ny, internal, bc_x, bc_y, u, v, p, &
          uold, vold, pold, unew, vnew, pnew, stream) bind(C, name="dlesm_shallow_step_sw_smooth_periodic_f64") result(rc)
       import :: c_int, c_ptr, c_sw_params, c_region, c_double
       type(c_sw_params), intent(in) :: params
       real(c_double), value :: alpha
       integer(c_int), value :: ld, ny, bc_x, bc_y
       type(c_region), intent(in) :: internal
       type(c_ptr), value :: u, v, p, uold, vold, pold, unew, vnew, pnew, stream
       integer(c_int) :: rc
     end function
     function dlesm_shallow_step_smooth_dm(plan, params, alpha, ld, ny, xstart, xstop, ystart, ystop, u, v, p, &
          uold, vold, pold, unew, vnew, pnew, stream) bind(C, name="dlesm_shallow_step_smooth_dm") result(rc)
       import :: c_int, c_ptr, c_sw_params, c_double
       type(c_ptr), value :: plan
       type(c_sw_params), intent(in) :: params
       real(c_double), value :: alpha
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: u, v, p, uold, vold, pold, unew, vnew, pnew, stream
       integer(c_int) :: rc
     end function
     function dlesm_shallow_step_smooth_dm_pipelined(plan, params, alpha, ld, ny, xstart, xstop, ystart, ystop, u, v, p, &
          uold, vold, pold, unew, vnew, pnew, stream) bind(C, name="dlesm_shallow_step_smooth_dm_pipelined") result(rc)
       import :: c_int, c_ptr, c_sw_params, c_double
       type(c_ptr), value :: plan
       type(c_sw_params), intent(in) :: params
       real(c_double), value :: alpha
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: u, v, p, uold, vold, pold, unew, vnew, pnew, stream
       integer(c_int) :: rc
     end function
     function dlesm_shallow_autotune_sw_f64(params, ld, ny, xstart, xstop, ystart, ystop, u, v, p, &
          uold, vold, pold, unew, vnew, pnew, stream) bind(C, name="dlesm_shallow_autotune_sw_f64") result(rc)
       import :: c_int, c_ptr, c_sw_params
       type(c_sw_params), intent(in) :: params
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: u, v, p, uold, vold, pold, unew, vnew, pnew, stream
       integer(c_int) :: rc
     end function
     ! the GOcean `shallow` kernels one by one (one launch per PSy loop nest); arrays in the kernels' own order
     function dlesm_compute_cu_f64(offset, ld, ny, xstart, xstop, ystart, ystop, cu, p, u, stream) &
          bind(C, name="dlesm_compute_cu_f64") result(rc)
       import :: c_int, c_ptr
       integer(c_int), value :: offset, ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: cu, p, u, stream
       integer(c_int) :: rc
     end function
     function dlesm_compute_cv_f64(offset, ld, ny, xstart, xstop, ystart, ystop, cv, p, v, stream) &
          bind(C, name="dlesm_compute_cv_f64") result(rc)
       import :: c_int, c_ptr
       integer(c_int), value :: offset, ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: cv, p, v, stream
       integer(c_int) :: rc
     end function
     function dlesm_compute_z_f64(offset, ld, ny, xstart, xstop, ystart, ystop, fsdx, fsdy, z, p, u, v, stream) &
          bind(C, name="dlesm_compute_z_f64") result(rc)
       import :: c_int, c_ptr, c_double
       integer(c_int), value :: offset, ld, ny, xstart, xstop, ystart, ystop
       real(c_double), value :: fsdx, fsdy
       type(c_ptr), value :: z, p, u, v, stream
       integer(c_int) :: rc
     end function
     function dlesm_compute_h_f64(offset, ld, ny, xstart, xstop, ystart, ystop, h, p, u, v, stream) &
          bind(C, name="dlesm_compute_h_f64") result(rc)
       import :: c_int, c_ptr
       integer(c_int), value :: offset, ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: h, p, u, v, stream
       integer(c_int) :: rc
     end function
     function dlesm_compute_unew_f64(offset, ld, ny, xstart, xstop, ystart, ystop, tdts8, tdtsdx, unew, uold, z, cv, &
          h, stream) bind(C, name="dlesm_compute_unew_f64") result(rc)
       import :: c_int, c_ptr, c_double
       integer(c_int), value :: offset, ld, ny, xstart, xstop, ystart, ystop
       real(c_double), value :: tdts8, tdtsdx
       type(c_ptr), value :: unew, uold, z, cv, h, stream
       integer(c_int) :: rc
     end function
     function dlesm_compute_vnew_f64(offset, ld, ny, xstart, xstop, ystart, ystop, tdts8, tdtsdy, vnew, vold, z, cu, &
          h, stream) bind(C, name="dlesm_compute_vnew_f64") result(rc)
       import :: c_int, c_ptr, c_double
       integer(c_int), value :: offset, ld, ny, xstart, xstop, ystart, ystop
       real(c_double), value :: tdts8, tdtsdy
       type(c_ptr), value :: vnew, vold, z, cu, h, stream
       integer(c_int) :: rc
     end function
     function dlesm_compute_pnew_f64(offset, ld, ny, xstart, xstop, ystart, ystop, tdtsdx, tdtsdy, pnew, pold, cu, cv, &
          stream) bind(C, name="dlesm_compute_pnew_f64") result(rc)
       import :: c_int, c_ptr, c_double
       integer(c_int), value :: offset, ld, ny, xstart, xstop, ystart, ystop
       real(c_double), value :: tdtsdx, tdtsdy
       type(c_ptr), value :: pnew, pold, cu, cv, stream
       integer(c_int) :: rc
     end function
     function dlesm_time_smooth_f64(ld, ny, xstart, xstop, ystart, ystop, alpha, field, field_new, field_old, stream) &
          bind(C, name="dlesm_time_smooth_f64") result(rc)
       import :: c_int, c_ptr, c_double
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       real(c_double), value :: alpha
       type(c_ptr), value :: field, field_new, field_old, stream
       integer(c_int) :: rc
     end function
     function dlesm_periodic_halos_apply_multi_f64(fields, nfields, ld, ny, internal, bc_x, bc_y, stream) &
          bind(C, name="dlesm_periodic_halos_apply_multi_f64") result(rc)
       import :: c_int, c_ptr, c_region
       type(c_ptr), intent(in) :: fields(*)
       integer(c_int), value :: nfields, ld, ny, bc_x, bc_y
       type(c_region), intent(in) :: internal
       type(c_ptr), value :: stream
       integer(c_int) :: rc
     end function
     function dlesm_periodic_halos_apply_f64(field, ld, ny, internal, bc_x, bc_y, stream) &
          bind(C, name="dlesm_periodic_halos_apply_f64") result(rc)
       import :: c_int, c_ptr, c_region
       type(c_ptr), value :: field, stream
       integer(c_int), value :: ld, ny, bc_x, bc_y
       type(c_region), intent(in) :: internal
       integer(c_int) :: rc
     end function
     function dlesm_shallow_autotune_f64(params, ld, ny, xstart, xstop, ystart, ystop, u, v, p, &
          uold, vold, pold, unew, vnew, pnew, stream) bind(C, name="dlesm_shallow_autotune_f64") result(rc)
       import :: c_int, c_ptr, c_sw_params
       type(c_sw_params), intent(in) :: params
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: u, v, p, uold, vold, pold, unew, vnew, pnew, stream
       integer(c_int) :: rc
     end function
     function dlesm_copy_patch_f64(src, dst, ld, ny_arr, sx0, sy0, dx0, dy0, nx, ny, stream) &
          bind(C, name="dlesm_copy_patch_f64") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: src, dst, stream
       integer(c_int), value :: ld, ny_arr, sx0, sy0, dx0, dy0, nx, ny
       integer(c_int) :: rc
     end function
     function dlesm_fill_f64(f, ld, ny, xstart, xstop, ystart, ystop, val, stream) &
          bind(C, name="dlesm_fill_f64") result(rc)
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: f, stream
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       real(c_double), value :: val
       integer(c_int) :: rc
     end function
     function dlesm_checksum_f64(f, ld, ny, xstart, xstop, ystart, ystop, res, stream) &
          bind(C, name="dlesm_checksum_f64") result(rc)
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: f, stream
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       real(c_double), intent(out) :: res
       integer(c_int) :: rc
     end function
     function dlesm_field_stats_async_f64(fields, masks, boxes, nfields, ld, ny, result_dev, stream) &
          bind(C, name="dlesm_field_stats_async_f64") result(rc)
       import :: c_int, c_ptr, c_region
       type(c_ptr), intent(in) :: fields(*)
       type(c_ptr), value :: masks           ! NULL, or the address of nfields mask pointers
       type(c_region), intent(in) :: boxes(*)
       integer(c_int), value :: nfields, ld, ny
       type(c_ptr), value :: result_dev, stream
       integer(c_int) :: rc
     end function
     function dlesm_field_stats_f64(fields, masks, boxes, nfields, ld, ny, result_host, stream) &
          bind(C, name="dlesm_field_stats_f64") result(rc)
       import :: c_int, c_ptr, c_region, field_stats_type
       type(c_ptr), intent(in) :: fields(*)
       type(c_ptr), value :: masks
       type(c_region), intent(in) :: boxes(*)
       integer(c_int), value :: nfields, ld, ny
       type(field_stats_type), intent(out) :: result_host(*)
       type(c_ptr), value :: stream
       integer(c_int) :: rc
     end function
     function dlesm_field_locate_f64(f, mask, ld, ny, xstart, xstop, ystart, ystop, what, val, index_host, stream) &
          bind(C, name="dlesm_field_locate_f64") result(rc)
       import :: c_int, c_ptr, c_double, c_int64_t
       type(c_ptr), value :: f, mask, stream
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop, what
       real(c_double), value :: val
       integer(c_int64_t), intent(out) :: index_host
       integer(c_int) :: rc
     end function
     function dlesm_hash_init_f64(f, ld, ny, xstart, xstop, ystart, ystop, seed, gx0, gy0, stream) &
          bind(C, name="dlesm_hash_init_f64") result(rc)
       import :: c_int, c_ptr, c_int64_t
       type(c_ptr), value :: f, stream
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       integer(c_int64_t), value :: seed, gx0, gy0
       integer(c_int) :: rc
     end function
     ! ---- halo exchange ------------------------------------------------------
     function dlesm_comm_unique_id(id) bind(C, name="dlesm_comm_unique_id") result(rc)
       import :: c_int, c_char
       character(kind=c_char), intent(out) :: id(*)
       integer(c_int) :: rc
     end function
     function dlesm_rendezvous_remove(path) bind(C, name="dlesm_rendezvous_remove") result(rc)
       import :: c_int, c_char
       character(kind=c_char), intent(in) :: path(*)
       integer(c_int) :: rc
     end function
     function dlesm_rendezvous_publish(path, id, token) bind(C, name="dlesm_rendezvous_publish") result(rc)
       import :: c_int, c_char
       character(kind=c_char), intent(in) :: path(*), id(*), token(*)
       integer(c_int) :: rc
     end function
     function dlesm_rendezvous_fetch(path, id, token, timeout_ms) &
          bind(C, name="dlesm_rendezvous_fetch") result(rc)
       import :: c_int, c_char
       character(kind=c_char), intent(in) :: path(*), token(*)
       character(kind=c_char), intent(out) :: id(*)
       integer(c_int), value :: timeout_ms
       integer(c_int) :: rc
     end function
     function dlesm_rendezvous_ack(path, rank0) bind(C, name="dlesm_rendezvous_ack") result(rc)
       import :: c_int, c_char
       character(kind=c_char), intent(in) :: path(*)
       integer(c_int), value :: rank0
       integer(c_int) :: rc
     end function
     function dlesm_rendezvous_wait_acks(path, nranks, timeout_ms) &
          bind(C, name="dlesm_rendezvous_wait_acks") result(rc)
       import :: c_int, c_char
       character(kind=c_char), intent(in) :: path(*)
       integer(c_int), value :: nranks, timeout_ms
       integer(c_int) :: rc
     end function
     function dlesm_comm_init(id, nranks, rank0) bind(C, name="dlesm_comm_init") result(rc)
       import :: c_int, c_char
       character(kind=c_char), intent(in) :: id(*)
       integer(c_int), value :: nranks, rank0
       integer(c_int) :: rc
     end function
     ! mailbox mode: no RCCL communicator (the session name is made by rank 0 and handed round like an RCCL id)
     function dlesm_board_nonce(id) bind(C, name="dlesm_board_nonce") result(rc)
       import :: c_int, c_char
       character(kind=c_char), intent(out) :: id(*)
       integer(c_int) :: rc
     end function
     function dlesm_board_abort(msg) bind(C, name="dlesm_board_abort") result(rc)
       import :: c_int, c_char
       character(kind=c_char), intent(in) :: msg(*)
       integer(c_int) :: rc
     end function
     function dlesm_comm_init_mailbox(id, nranks, rank0) bind(C, name="dlesm_comm_init_mailbox") result(rc)
       import :: c_int, c_char
       character(kind=c_char), intent(in) :: id(*)
       integer(c_int), value :: nranks, rank0
       integer(c_int) :: rc
     end function
     function dlesm_comm_finalize() bind(C, name="dlesm_comm_finalize") result(rc)
       import :: c_int
       integer(c_int) :: rc
     end function
     function dlesm_halo_plan_create(tables, ld, ny, plan) &
          bind(C, name="dlesm_halo_plan_create") result(rc)
       import :: c_int, c_ptr, c_comm_tables
       type(c_comm_tables), intent(in) :: tables
       integer(c_int), value :: ld, ny
       type(c_ptr), intent(out) :: plan
       integer(c_int) :: rc
     end function
     function dlesm_halo_plan_destroy(plan) bind(C, name="dlesm_halo_plan_destroy") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: plan
       integer(c_int) :: rc
     end function
     function dlesm_halo_exchange_f64(plan, field, dirs_mask, stream) &
          bind(C, name="dlesm_halo_exchange_f64") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: plan, field, stream
       integer(c_int), value :: dirs_mask
       integer(c_int) :: rc
     end function
     function dlesm_jacobi5_step_dm(plan, in, out, ld, ny, xstart, xstop, ystart, ystop, stream) &
          bind(C, name="dlesm_jacobi5_step_dm") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: plan, in, out, stream
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       integer(c_int) :: rc
     end function
     function dlesm_stencil5_autotune_f64(in, out, ld, ny, xstart, xstop, ystart, ystop, stream) &
          bind(C, name="dlesm_stencil5_autotune_f64") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: in, out, stream
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       integer(c_int) :: rc
     end function
     function dlesm_stencil5_multi_f64(in, out, ld, ny, nsteps, xstart, xstop, ystart, ystop, &
          exstart, exstop, eystart, eystop, grow_w, grow_e, grow_s, grow_n, stream) &
          bind(C, name="dlesm_stencil5_multi_f64") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: in, out, stream
       integer(c_int), value :: ld, ny, nsteps, xstart, xstop, ystart, ystop
       integer(c_int), value :: exstart, exstop, eystart, eystop, grow_w, grow_e, grow_s, grow_n
       integer(c_int) :: rc
     end function
     function dlesm_jacobi5_step_dm_pipelined(plan, in, out, ld, ny, xstart, xstop, ystart, ystop, stream) &
          bind(C, name="dlesm_jacobi5_step_dm_pipelined") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: plan, in, out, stream
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       integer(c_int) :: rc
     end function
     function dlesm_halo_plan_join(plan, stream) bind(C, name="dlesm_halo_plan_join") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: plan, stream
       integer(c_int) :: rc
     end function
     ! peer transport: connect the plan to the neighbours' mailboxes (collective; the blobs travel by ncclAllGather)
     function dlesm_halo_plan_peer_connect_rccl(plan, nfields) bind(C, name="dlesm_halo_plan_peer_connect_rccl") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: plan
       integer(c_int), value :: nfields
       integer(c_int) :: rc
     end function
     function dlesm_halo_plan_peer_connected(plan) bind(C, name="dlesm_halo_plan_peer_connected") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: plan
       integer(c_int) :: rc
     end function
     function dlesm_jacobi5_multi_step_dm(plan, in, out, ld, ny, nsteps, xstart, xstop, ystart, ystop, &
          stream) bind(C, name="dlesm_jacobi5_multi_step_dm") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: plan, in, out, stream
       integer(c_int), value :: ld, ny, nsteps, xstart, xstop, ystart, ystop
       integer(c_int) :: rc
     end function
     function dlesm_halo_exchange_multi_f64(plan, fields, nfields, dirs_mask, stream) &
          bind(C, name="dlesm_halo_exchange_multi_f64") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: plan, stream
       type(c_ptr), intent(in) :: fields(*)
       integer(c_int), value :: nfields, dirs_mask
       integer(c_int) :: rc
     end function
     function dlesm_shallow_step_dm(plan, params, ld, ny, xstart, xstop, ystart, ystop, u, v, p, &
          uold, vold, pold, unew, vnew, pnew, stream) bind(C, name="dlesm_shallow_step_dm") result(rc)
       import :: c_int, c_ptr, c_sw_params
       type(c_ptr), value :: plan
       type(c_sw_params), intent(in) :: params
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: u, v, p, uold, vold, pold, unew, vnew, pnew, stream
       integer(c_int) :: rc
     end function
     function dlesm_nemolite_step_dm(plan, params, grid, area_t, ld, ny, tbox, ubox, vbox, obc, ssh_bc, un, vn, ht, hu, hv, &
          sshn_t, sshn_u, sshn_v, ssha, ssha_u, ssha_v, ua, va, stream) bind(C, name="dlesm_nemolite_step_dm") result(rc)
       import :: c_int, c_ptr, c_double, c_momentum_params, c_momentum_grid, c_region
       type(c_ptr), value :: plan
       type(c_momentum_params), intent(in) :: params
       type(c_momentum_grid), intent(in) :: grid
       type(c_ptr), value :: area_t
       integer(c_int), value :: ld, ny
       type(c_region), intent(in) :: tbox, ubox, vbox
       type(c_ptr), value :: obc
       real(c_double), value :: ssh_bc
       type(c_ptr), value :: un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, ssha, ssha_u, ssha_v, ua, va, stream
       integer(c_int) :: rc
     end function
     function dlesm_nemolite_step_wet_dm(plan, wet, params, grid, area_t, ld, ny, tbox, ubox, vbox, obc, ssh_bc, un, vn, ht, &
          hu, hv, sshn_t, sshn_u, sshn_v, ssha, ssha_u, ssha_v, ua, va, stream) bind(C, name="dlesm_nemolite_step_wet_dm") &
          result(rc)
       import :: c_int, c_ptr, c_double, c_momentum_params, c_momentum_grid, c_region
       type(c_ptr), value :: plan, wet
       type(c_momentum_params), intent(in) :: params
       type(c_momentum_grid), intent(in) :: grid
       type(c_ptr), value :: area_t
       integer(c_int), value :: ld, ny
       type(c_region), intent(in) :: tbox, ubox, vbox
       type(c_ptr), value :: obc
       real(c_double), value :: ssh_bc
       type(c_ptr), value :: un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, ssha, ssha_u, ssha_v, ua, va, stream
       integer(c_int) :: rc
     end function
     ! ---- tracer transport (DESIGN.md section 6.10): c_in, c_out = host arrays of ntracers device pointers
     function dlesm_tracer_step_f64(rdt, ld, ny, xstart, xstop, ystart, ystop, tmask, area_t, un, vn, hu, hv, ht, sshn_t, &
          sshn_u, sshn_v, ssha, c_in, c_out, ntracers, stream) bind(C, name="dlesm_tracer_step_f64") result(rc)
       import :: c_int, c_ptr, c_double
       real(c_double), value :: rdt
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, ssha
       type(c_ptr), intent(in) :: c_in(*), c_out(*)
       integer(c_int), value :: ntracers
       type(c_ptr), value :: stream
       integer(c_int) :: rc
     end function
     function dlesm_tracer_step_dm(plan, rdt, ld, ny, xstart, xstop, ystart, ystop, tmask, area_t, un, vn, hu, hv, ht, &
          sshn_t, sshn_u, sshn_v, ssha, c_in, c_out, ntracers, stream) bind(C, name="dlesm_tracer_step_dm") result(rc)
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: plan
       real(c_double), value :: rdt
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, ssha
       type(c_ptr), intent(in) :: c_in(*), c_out(*)
       integer(c_int), value :: ntracers
       type(c_ptr), value :: stream
       integer(c_int) :: rc
     end function
     ! ---- second-order limited tracer transport (DESIGN.md section 6.11): the same argument lists
     function dlesm_tracer_step_muscl_f64(rdt, ld, ny, xstart, xstop, ystart, ystop, tmask, area_t, un, vn, hu, hv, ht, sshn_t, &
          sshn_u, sshn_v, ssha, c_in, c_out, ntracers, stream) bind(C, name="dlesm_tracer_step_muscl_f64") result(rc)
       import :: c_int, c_ptr, c_double
       real(c_double), value :: rdt
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, ssha
       type(c_ptr), intent(in) :: c_in(*), c_out(*)
       integer(c_int), value :: ntracers
       type(c_ptr), value :: stream
       integer(c_int) :: rc
     end function
     function dlesm_tracer_step_muscl_dm(plan, rdt, ld, ny, xstart, xstop, ystart, ystop, tmask, area_t, un, vn, hu, hv, ht, &
          sshn_t, sshn_u, sshn_v, ssha, c_in, c_out, ntracers, stream) bind(C, name="dlesm_tracer_step_muscl_dm") result(rc)
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: plan
       real(c_double), value :: rdt
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, ssha
       type(c_ptr), intent(in) :: c_in(*), c_out(*)
       integer(c_int), value :: ntracers
       type(c_ptr), value :: stream
       integer(c_int) :: rc
     end function
     ! ---- time-centred limited tracer transport (DESIGN.md section 6.12): the same argument lists
     function dlesm_tracer_step_hancock_f64(rdt, ld, ny, xstart, xstop, ystart, ystop, tmask, area_t, un, vn, hu, hv, ht, sshn_t, &
          sshn_u, sshn_v, ssha, c_in, c_out, ntracers, stream) bind(C, name="dlesm_tracer_step_hancock_f64") result(rc)
       import :: c_int, c_ptr, c_double
       real(c_double), value :: rdt
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, ssha
       type(c_ptr), intent(in) :: c_in(*), c_out(*)
       integer(c_int), value :: ntracers
       type(c_ptr), value :: stream
       integer(c_int) :: rc
     end function
     function dlesm_tracer_step_hancock_dm(plan, rdt, ld, ny, xstart, xstop, ystart, ystop, tmask, area_t, un, vn, hu, hv, ht, &
          sshn_t, sshn_u, sshn_v, ssha, c_in, c_out, ntracers, stream) bind(C, name="dlesm_tracer_step_hancock_dm") result(rc)
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: plan
       real(c_double), value :: rdt
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, ssha
       type(c_ptr), intent(in) :: c_in(*), c_out(*)
       integer(c_int), value :: ntracers
       type(c_ptr), value :: stream
       integer(c_int) :: rc
     end function
     ! ---- the tracer schemes' Courant check (DESIGN.md section 6.14): the flow arrays of the tracer entries without ssha
     function dlesm_tracer_courant_async_f64(rdt, ld, ny, xstart, xstop, ystart, ystop, tmask, area_t, un, vn, hu, hv, ht, sshn_t, &
          sshn_u, sshn_v, face_limit, outflow_limit, result_dev, stream) bind(C, name="dlesm_tracer_courant_async_f64") result(rc)
       import :: c_int, c_ptr, c_double
       real(c_double), value :: rdt
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v
       real(c_double), value :: face_limit, outflow_limit
       type(c_ptr), value :: result_dev, stream
       integer(c_int) :: rc
     end function
     function dlesm_tracer_courant_f64(rdt, ld, ny, xstart, xstop, ystart, ystop, tmask, area_t, un, vn, hu, hv, ht, sshn_t, &
          sshn_u, sshn_v, face_limit, outflow_limit, result_host, stream) bind(C, name="dlesm_tracer_courant_f64") result(rc)
       import :: c_int, c_ptr, c_double, tracer_courant_type
       real(c_double), value :: rdt
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v
       real(c_double), value :: face_limit, outflow_limit
       type(tracer_courant_type), intent(out) :: result_host
       type(c_ptr), value :: stream
       integer(c_int) :: rc
     end function
     ! ---- the flow step's own stability check (DESIGN.md section 6.15)
     function dlesm_flow_courant_async_f64(rdt, g, visc, ld, ny, xstart, xstop, ystart, ystop, tmask, dx_t, dy_t, un, vn, ht, &
          sshn_t, gravity_limit, advective_limit, viscous_limit, depth_limit, &
          result_dev, stream) bind(C, name="dlesm_flow_courant_async_f64") result(rc)
       import :: c_int, c_ptr, c_double
       real(c_double), value :: rdt, g, visc
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: tmask, dx_t, dy_t, un, vn, ht, sshn_t
       real(c_double), value :: gravity_limit, advective_limit, viscous_limit, depth_limit
       type(c_ptr), value :: result_dev, stream
       integer(c_int) :: rc
     end function
     function dlesm_flow_courant_f64(rdt, g, visc, ld, ny, xstart, xstop, ystart, ystop, tmask, dx_t, dy_t, un, vn, ht, &
          sshn_t, gravity_limit, advective_limit, viscous_limit, depth_limit, &
          result_host, stream) bind(C, name="dlesm_flow_courant_f64") result(rc)
       import :: c_int, c_ptr, c_double, flow_courant_type
       real(c_double), value :: rdt, g, visc
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: tmask, dx_t, dy_t, un, vn, ht, sshn_t
       real(c_double), value :: gravity_limit, advective_limit, viscous_limit, depth_limit
       type(flow_courant_type), intent(out) :: result_host
       type(c_ptr), value :: stream
       integer(c_int) :: rc
     end function
     ! ---- the model's output fields (DESIGN.md section 6.16): mode 0 stores, 1 adds weight * value; out: six device pointers
     !      in the order SSH, UT, VT, SPEED, KE, VORT, c_null_ptr = not wanted
     function dlesm_flow_output_f64(mode, weight, ld, ny, xstart, xstop, ystart, ystop, tmask, dx_v, dy_u, un, vn, ht, &
          sshn_t, out, stream) bind(C, name="dlesm_flow_output_f64") result(rc)
       import :: c_int, c_ptr, c_double
       integer(c_int), value :: mode
       real(c_double), value :: weight
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: tmask, dx_v, dy_u, un, vn, ht, sshn_t
       type(c_ptr), intent(in) :: out(*)
       type(c_ptr), value :: stream
       integer(c_int) :: rc
     end function
     ! ---- drifters (DESIGN.md section 6.17): particles carried through the level-n flow, status 0 ACTIVE, 1 LEFT, 2 OPEN,
     !      3 GROUNDED; px, py, status: device arrays of n elements (dlesm_drifters_arrays gives those of a set)
     function dlesm_drifter_step_f64(h, nsub, ld, ny, xstart, xstop, ystart, ystop, tmask, dx_t, dy_t, un, vn, n, px, py, &
          status, stream) bind(C, name="dlesm_drifter_step_f64") result(rc)
       import :: c_int, c_ptr, c_double, c_long_long
       real(c_double), value :: h
       integer(c_int), value :: nsub, ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: tmask, dx_t, dy_t, un, vn
       integer(c_long_long), value :: n
       type(c_ptr), value :: px, py, status, stream
       integer(c_int) :: rc
     end function
     function dlesm_drifter_sample_f64(ld, ny, xstart, xstop, ystart, ystop, n, px, py, status, fields, out, nfields, &
          stream) bind(C, name="dlesm_drifter_sample_f64") result(rc)
       import :: c_int, c_ptr, c_long_long
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       integer(c_long_long), value :: n
       type(c_ptr), value :: px, py, status
       type(c_ptr), intent(in) :: fields(*), out(*)
       integer(c_int), value :: nfields
       type(c_ptr), value :: stream
       integer(c_int) :: rc
     end function
     ! the owner of the three arrays: create (status zeroed = all ACTIVE), put host -> device (status c_null_ptr = all
     ! ACTIVE), get device -> host after waiting (c_null_ptr = skip), arrays (the device pointers), destroy
     function dlesm_drifters_create(n, set) bind(C, name="dlesm_drifters_create") result(rc)
       import :: c_int, c_ptr, c_long_long
       integer(c_long_long), value :: n
       type(c_ptr), intent(out) :: set
       integer(c_int) :: rc
     end function
     function dlesm_drifters_put(set, px, py, status) bind(C, name="dlesm_drifters_put") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: set, px, py, status
       integer(c_int) :: rc
     end function
     function dlesm_drifters_get(set, px, py, status) bind(C, name="dlesm_drifters_get") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: set, px, py, status
       integer(c_int) :: rc
     end function
     function dlesm_drifters_arrays(set, n, px, py, status) bind(C, name="dlesm_drifters_arrays") result(rc)
       import :: c_int, c_ptr, c_long_long
       type(c_ptr), value :: set
       integer(c_long_long), intent(out) :: n
       type(c_ptr), intent(out) :: px, py, status
       integer(c_int) :: rc
     end function
     function dlesm_drifters_destroy(set) bind(C, name="dlesm_drifters_destroy") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: set
       integer(c_int) :: rc
     end function
     ! ---- particles in cell order (DESIGN.md section 6.18): perm = the stable ascending order of the particles' cell keys,
     !      the live ones in front (nlive: one int on the device, c_null_ptr = not wanted); the gather dst = src(perm) of 1..8
     !      arrays of 4- or 8-byte elements; both for the owner, which keeps origin; origin and nlive on the host after waiting
     function dlesm_particle_order_scratch(n, bytes) bind(C, name="dlesm_particle_order_scratch") result(rc)
       import :: c_int, c_long_long
       integer(c_long_long), value :: n
       integer(c_long_long), intent(out) :: bytes
       integer(c_int) :: rc
     end function
     function dlesm_particle_order_f64(xstart, xstop, ystart, ystop, n, px, py, status, perm, nlive, scratch, scratch_bytes, &
          stream) bind(C, name="dlesm_particle_order_f64") result(rc)
       import :: c_int, c_ptr, c_long_long
       integer(c_int), value :: xstart, xstop, ystart, ystop
       integer(c_long_long), value :: n
       type(c_ptr), value :: px, py, status, perm, nlive, scratch
       integer(c_long_long), value :: scratch_bytes
       type(c_ptr), value :: stream
       integer(c_int) :: rc
     end function
     function dlesm_particle_permute(n, perm, narrays, src, dst, elem_bytes, &
          stream) bind(C, name="dlesm_particle_permute") result(rc)
       import :: c_int, c_ptr, c_long_long
       integer(c_long_long), value :: n
       type(c_ptr), value :: perm
       integer(c_int), value :: narrays
       type(c_ptr), intent(in) :: src(*), dst(*)
       integer(c_int), intent(in) :: elem_bytes(*)
       type(c_ptr), value :: stream
       integer(c_int) :: rc
     end function
     function dlesm_particle_sort_set(set, xstart, xstop, ystart, ystop, &
          stream) bind(C, name="dlesm_particle_sort_set") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: set
       integer(c_int), value :: xstart, xstop, ystart, ystop
       type(c_ptr), value :: stream
       integer(c_int) :: rc
     end function
     function dlesm_particle_set_origin(set, origin, nlive) bind(C, name="dlesm_particle_set_origin") result(rc)
       import :: c_int, c_ptr, c_long_long
       type(c_ptr), value :: set, origin
       integer(c_long_long), intent(out) :: nlive
       integer(c_int) :: rc
     end function
     ! ---- particles binned by cell (DESIGN.md section 6.19): per-cell sums of 1..8 per-particle weights (c_null_ptr: the
     !      count) over a permutation in key order (perm = c_null_ptr: the identity) into T-point arrays, mode 0 stores
     !      alpha * sum in every cell of the box, mode 1 adds it where a live particle is; unordered: one int on the device
     !      (c_null_ptr = not wanted); and the count for the owner
     function dlesm_cell_bin_scratch(n, narrays, bytes) bind(C, name="dlesm_cell_bin_scratch") result(rc)
       import :: c_int, c_long_long
       integer(c_long_long), value :: n
       integer(c_int), value :: narrays
       integer(c_long_long), intent(out) :: bytes
       integer(c_int) :: rc
     end function
     function dlesm_cell_bin_f64(mode, alpha, ld, ny, xstart, xstop, ystart, ystop, n, px, py, status, perm, narrays, &
          weights, out, unordered, scratch, scratch_bytes, stream) bind(C, name="dlesm_cell_bin_f64") result(rc)
       import :: c_int, c_ptr, c_double, c_long_long
       integer(c_int), value :: mode
       real(c_double), value :: alpha
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       integer(c_long_long), value :: n
       type(c_ptr), value :: px, py, status, perm
       integer(c_int), value :: narrays
       type(c_ptr), intent(in) :: weights(*), out(*)
       type(c_ptr), value :: unordered, scratch
       integer(c_long_long), value :: scratch_bytes
       type(c_ptr), value :: stream
       integer(c_int) :: rc
     end function
     function dlesm_cell_bin_set(set, mode, alpha, ld, ny, xstart, xstop, ystart, ystop, count, &
          stream) bind(C, name="dlesm_cell_bin_set") result(rc)
       import :: c_int, c_ptr, c_double
       type(c_ptr), value :: set
       integer(c_int), value :: mode
       real(c_double), value :: alpha
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: count, stream
       integer(c_int) :: rc
     end function
     ! ---- drifters with random-walk diffusion (DESIGN.md section 6.20): section 6.17's step plus a Philox4x32-10 kick of
     !      variance 2 kh |h| per axis and substep, keyed by seed, counted by (id, tick + substep); id: device ints or
     !      c_null_ptr (the slot number), tick_dev: one device integer(c_long_long) added to tick and advanced by nsub, or
     !      c_null_ptr; and the step for the owner, whose origin is the id
     function dlesm_dispersal_step_f64(h, nsub, kh, seed, tick, tick_dev, ld, ny, xstart, xstop, ystart, ystop, tmask, dx_t, &
          dy_t, un, vn, n, id, px, py, status, stream) bind(C, name="dlesm_dispersal_step_f64") result(rc)
       import :: c_int, c_ptr, c_double, c_long_long
       real(c_double), value :: h
       integer(c_int), value :: nsub
       real(c_double), value :: kh
       integer(c_long_long), value :: seed, tick
       type(c_ptr), value :: tick_dev
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: tmask, dx_t, dy_t, un, vn
       integer(c_long_long), value :: n
       type(c_ptr), value :: id, px, py, status, stream
       integer(c_int) :: rc
     end function
     function dlesm_dispersal_step_set(set, h, nsub, kh, seed, tick, tick_dev, ld, ny, xstart, xstop, ystart, ystop, tmask, &
          dx_t, dy_t, un, vn, stream) bind(C, name="dlesm_dispersal_step_set") result(rc)
       import :: c_int, c_ptr, c_double, c_long_long
       type(c_ptr), value :: set
       real(c_double), value :: h
       integer(c_int), value :: nsub
       real(c_double), value :: kh
       integer(c_long_long), value :: seed, tick
       type(c_ptr), value :: tick_dev
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: tmask, dx_t, dy_t, un, vn, stream
       integer(c_int) :: rc
     end function
     ! ---- drifters in a varying diffusivity (DESIGN.md section 6.22): section 6.20's step with the kick made from the T-point
     !      field kh_t (device doubles laid out like dx_t) and Visser's drift correction; everything else as above
     function dlesm_random_walk_f64(h, nsub, kh_t, seed, tick, tick_dev, ld, ny, xstart, xstop, ystart, ystop, tmask, dx_t, &
          dy_t, un, vn, n, id, px, py, status, stream) bind(C, name="dlesm_random_walk_f64") result(rc)
       import :: c_int, c_ptr, c_double, c_long_long
       real(c_double), value :: h
       integer(c_int), value :: nsub
       type(c_ptr), value :: kh_t
       integer(c_long_long), value :: seed, tick
       type(c_ptr), value :: tick_dev
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: tmask, dx_t, dy_t, un, vn
       integer(c_long_long), value :: n
       type(c_ptr), value :: id, px, py, status, stream
       integer(c_int) :: rc
     end function
     function dlesm_random_walk_set(set, h, nsub, kh_t, seed, tick, tick_dev, ld, ny, xstart, xstop, ystart, ystop, tmask, &
          dx_t, dy_t, un, vn, stream) bind(C, name="dlesm_random_walk_set") result(rc)
       import :: c_int, c_ptr, c_double, c_long_long
       type(c_ptr), value :: set
       real(c_double), value :: h
       integer(c_int), value :: nsub
       type(c_ptr), value :: kh_t
       integer(c_long_long), value :: seed, tick
       type(c_ptr), value :: tick_dev
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: tmask, dx_t, dy_t, un, vn, stream
       integer(c_int) :: rc
     end function
     ! ---- the coupled step on a decomposed grid and the int halo exchange (DESIGN.md section 6.13)
     function dlesm_nemolite_coupled_step_dm(plan, wet, scheme, params, grid, area_t, ld, ny, tbox, ubox, vbox, obc, ssh_bc, un, &
          vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, ssha, ssha_u, ssha_v, ua, va, c_in, c_out, ntracers, stream) &
          bind(C, name="dlesm_nemolite_coupled_step_dm") result(rc)
       import :: c_int, c_ptr, c_double, c_momentum_params, c_momentum_grid, c_region
       type(c_ptr), value :: plan, wet
       integer(c_int), value :: scheme
       type(c_momentum_params), intent(in) :: params
       type(c_momentum_grid), intent(in) :: grid
       type(c_ptr), value :: area_t
       integer(c_int), value :: ld, ny
       type(c_region), intent(in) :: tbox, ubox, vbox
       type(c_ptr), value :: obc
       real(c_double), value :: ssh_bc
       type(c_ptr), value :: un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, ssha, ssha_u, ssha_v, ua, va
       type(c_ptr), intent(in) :: c_in(*), c_out(*)
       integer(c_int), value :: ntracers
       type(c_ptr), value :: stream
       integer(c_int) :: rc
     end function
     function dlesm_halo_exchange_i32(plan, field, stream) bind(C, name="dlesm_halo_exchange_i32") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: plan, field, stream
       integer(c_int) :: rc
     end function
     function dlesm_shallow_step_x2_dm(plan, params, ld, ny, xstart, xstop, ystart, ystop, u, v, p, uold, vold, pold, &
          unew, vnew, pnew, unew2, vnew2, pnew2, stream) bind(C, name="dlesm_shallow_step_x2_dm") result(rc)
       import :: c_int, c_ptr, c_sw_params
       type(c_ptr), value :: plan
       type(c_sw_params), intent(in) :: params
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: u, v, p, uold, vold, pold, unew, vnew, pnew, unew2, vnew2, pnew2, stream
       integer(c_int) :: rc
     end function
     function dlesm_shallow_step_smooth_x2_dm(plan, params, alpha, ld, ny, xstart, xstop, ystart, ystop, u, v, p, uold, vold, &
          pold, unew2, vnew2, pnew2, uold2, vold2, pold2, stream) bind(C, name="dlesm_shallow_step_smooth_x2_dm") result(rc)
       import :: c_int, c_ptr, c_sw_params, c_double
       type(c_ptr), value :: plan
       type(c_sw_params), intent(in) :: params
       real(c_double), value :: alpha
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: u, v, p, uold, vold, pold, unew2, vnew2, pnew2, uold2, vold2, pold2, stream
       integer(c_int) :: rc
     end function
     function dlesm_shallow_step_dm_pipelined(plan, params, ld, ny, xstart, xstop, ystart, ystop, u, v, p, &
          uold, vold, pold, unew, vnew, pnew, stream) bind(C, name="dlesm_shallow_step_dm_pipelined") result(rc)
       import :: c_int, c_ptr, c_sw_params
       type(c_ptr), value :: plan
       type(c_sw_params), intent(in) :: params
       integer(c_int), value :: ld, ny, xstart, xstop, ystart, ystop
       type(c_ptr), value :: u, v, p, uold, vold, pold, unew, vnew, pnew, stream
       integer(c_int) :: rc
     end function
     function dlesm_global_sum_f64(val) bind(C, name="dlesm_global_sum_f64") result(rc)
       import :: c_int, c_double
       real(c_double), intent(inout) :: val
       integer(c_int) :: rc
     end function
     function dlesm_global_max_f64(val) bind(C, name="dlesm_global_max_f64") result(rc)
       import :: c_int, c_double
       real(c_double), intent(inout) :: val
       integer(c_int) :: rc
     end function
     function dlesm_gather_inner_f64(field, ld, ny, internal, decomp, subdomains, nranks, global_host) &
          bind(C, name="dlesm_gather_inner_f64") result(rc)
       import :: c_int, c_ptr, c_region, c_decomp, c_subdomain
       type(c_ptr), value :: field, global_host
       integer(c_int), value :: ld, ny, nranks
       type(c_region), intent(in) :: internal
       type(c_decomp), intent(in) :: decomp
       type(c_subdomain), intent(in) :: subdomains(*)
       integer(c_int) :: rc
     end function
     function dlesm_gather_f64(send, recv, n) bind(C, name="dlesm_gather_f64") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: send, recv
       integer(c_int), value :: n
       integer(c_int) :: rc
     end function
     ! ---- libc / HIP helpers the Fortran layer needs ---------------------------
     function c_strlen(s) bind(C, name="strlen") result(n)
       import :: c_ptr, c_size_t
       type(c_ptr), value :: s
       integer(c_size_t) :: n
     end function
     function hipDeviceSynchronize() bind(C, name="hipDeviceSynchronize") result(rc)
       import :: c_int
       integer(c_int) :: rc
     end function
     function hipMalloc(ptr, nbytes) bind(C, name="hipMalloc") result(rc)
       import :: c_int, c_ptr, c_size_t
       type(c_ptr), intent(out) :: ptr
       integer(c_size_t), value :: nbytes
       integer(c_int) :: rc
     end function
     function hipFree(ptr) bind(C, name="hipFree") result(rc)
       import :: c_int, c_ptr
       type(c_ptr), value :: ptr
       integer(c_int) :: rc
     end function
     function hipMemcpy(dst, src, nbytes, kind) bind(C, name="hipMemcpy") result(rc)
       import :: c_int, c_ptr, c_size_t
       type(c_ptr), value :: dst, src
       integer(c_size_t), value :: nbytes
       integer(c_int), value :: kind
       integer(c_int) :: rc
     end function
  end interface

contains

  !> Text of the library's last error as a Fortran string
  function dlesm_error_text() result(txt)
    character(len=:), allocatable :: txt
    type(c_ptr) :: p
    character(kind=c_char), pointer :: chars(:)
    integer :: n, i
    p = dlesm_last_error()
    if (.not. c_associated(p)) then
       txt = ''
       return
    end if
    n = int(c_strlen(p))
    call c_f_pointer(p, chars, [n])
    allocate(character(len=n) :: txt)
    do i = 1, n
       txt(i:i) = chars(i)
    end do
  end function dlesm_error_text

end module dlesm_hip_mod
