!> GPU test of the Fortran wrapper of the Jacobi step with its residual (tests/test_gpu_fortran_jacobi_residual.py).
!! One rank: a hash-filled input (with a few cells scaled up, so that the max is not everywhere alike), then
!! invoke_jacobi5_residual with norm 'max' into one output field and with 'l2' into another.  The extents, the internal
!! region, the input, both outputs and both returned values go to the file OUT (stream access, native byte order).
!! A norm that is neither must stop.  Mode "dm" (any number of ranks, tests/test_a_fortran_jacobi_residual_ranks_gpu.py): the
!! input is a function of the global cell index, and each rank prints the two values' bits and whether its `out` holds the
!! neighbours' cells in its depth-1 halos after the calls.
!!   ftest_jacobi_residual.exe NX NY run|badnorm|dm OUT
program ftest_jacobi_residual
  use iso_c_binding
  use kind_params_mod
  use parallel_mod
  use grid_mod
  use field_mod
  use gocean_mod
  use dlesm_psy_mod
  implicit none
  character(len=256) :: arg, mode, out
  integer :: nx, ny, i, j, u, ox, oy, bad
  type(grid_type), target :: g
  type(r2d_field), target :: fin, fmax, fl2, fchk
  real(go_wp) :: rmax, rl2

  call get_command_argument(1, arg); read(arg, *) nx
  call get_command_argument(2, arg); read(arg, *) ny
  call get_command_argument(3, mode)
  call get_command_argument(4, out)
  call gocean_initialise()
  g = grid_type(GO_ARAKAWA_C, (/GO_BC_EXTERNAL, GO_BC_EXTERNAL, GO_BC_NONE/), GO_OFFSET_NE)
  call g%decompose(nx, ny)
  call grid_init(g, 1.0_go_wp, 1.0_go_wp)
  fin = r2d_field(g, GO_T_POINTS)
  fmax = r2d_field(g, GO_T_POINTS)
  fl2 = r2d_field(g, GO_T_POINTS)
  call invoke_hash_init(fin, int(20261016, c_int64_t))
  call fin%read_from_device()
  ox = g%subdomain%global%xstart - g%subdomain%internal%xstart      ! local index + ox = global index
  oy = g%subdomain%global%ystart - g%subdomain%internal%ystart
  do j = 1, g%ny
     do i = 1, g%nx
        if (mod(3*(i + ox) + 5*(j + oy), 17) == 0) fin%data(i, j) = 40.0_go_wp * fin%data(i, j) - 20.0_go_wp
     end do
  end do
  call fin%write_to_device()

  if (trim(mode) == 'dm') then
     rmax = invoke_jacobi5_residual(fmax, fin, 'max')
     rl2 = invoke_jacobi5_residual(fl2, fin, 'l2')
     ! the halos the calls left against a halo exchange of a copy of the result
     call fmax%read_from_device()
     fchk = r2d_field(g, GO_T_POINTS)
     call invoke_copy(fchk, fmax)
     call fchk%halo_exchange(1)
     call fchk%read_from_device()
     bad = count(fchk%data /= fmax%data)
     write(*, '("G: rank ",I0," of ",I0," rmax ",Z16.16," rl2 ",Z16.16," halo cells differ ",I0)') get_rank(), &
          get_num_ranks(), transfer(real(rmax, c_double), 0_c_int64_t), transfer(real(rl2, c_double), 0_c_int64_t), bad
     call gocean_finalise()
     stop
  end if

  if (trim(mode) == 'badnorm') then
     rmax = invoke_jacobi5_residual(fmax, fin, 'linf')
     write(*, '("G: an unknown norm returned")')
     call gocean_finalise()
     stop
  end if

  rmax = invoke_jacobi5_residual(fmax, fin, 'max')
  rl2 = invoke_jacobi5_residual(fl2, fin, 'l2')
  call fmax%read_from_device()
  call fl2%read_from_device()
  open(newunit=u, file=trim(out), access='stream', form='unformatted', status='replace')
  write(u) int(g%nx, c_int), int(g%ny, c_int)
  write(u) int((/fmax%internal%xstart, fmax%internal%xstop, fmax%internal%ystart, fmax%internal%ystop/), c_int)
  write(u) fin%data, fmax%data, fl2%data
  write(u) real(rmax, c_double), real(rl2, c_double)
  close(u)
  write(*, '("G: residuals written")')
  call gocean_finalise()
end program ftest_jacobi_residual
