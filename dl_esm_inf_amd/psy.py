"""The "PSy layer" for the Python mirror: what PSyclone would generate around each kernel
(`do jj = fld%internal%ystart, ... ; do ji = ...; call kern_code(ji, jj, ...)`, form
infrastructure_mod.f90:32-41) becomes one launch of the matching HIP kernel over the same
index box."""
import collections
import ctypes as C
import math

from . import _cabi, grid_mod, parallel_mod
from ._cabi import SwParams, check
from .field_mod import GO_T_POINTS, _fetch_record, _stream_ptr, field_bounds


def invoke_jacobi5(out_fld, in_fld, stream=None):
    """out = 0.25*((w+e)+(s+n)) over out_fld%internal"""
    g, it = out_fld.grid, out_fld.internal
    check(_cabi.lib().dlesm_stencil5_f64(in_fld.device_ptr, out_fld.device_ptr, g.nx, g.ny,
                                         it.xstart, it.xstop, it.ystart, it.ystop,
                                         _stream_ptr(stream)))


def invoke_stencil9(out_fld, in_fld, coef, stream=None):
    """general 3x3 weighted stencil over out_fld%internal; coef: 9 weights, south-west row first
    (sw, s, se, w, c, e, nw, n, ne) or a 3x3 array indexed [dj+1][di+1]"""
    import numpy as np
    c = np.ascontiguousarray(np.asarray(coef, dtype=np.float64).reshape(9))
    g, it = out_fld.grid, out_fld.internal
    check(_cabi.lib().dlesm_stencil9_f64(in_fld.device_ptr, out_fld.device_ptr,
                                         c.ctypes.data_as(C.POINTER(C.c_double)), g.nx, g.ny,
                                         it.xstart, it.xstop, it.ystart, it.ystop, _stream_ptr(stream)))


def invoke_stencil9_dm(out_fld, in_fld, coef, stream=None):
    """distributed step of a 3x3 weighted kernel: frame, exchange(out) (eight directions when a
    corner weight is non-zero) beside the interior sweep, join"""
    import numpy as np
    c = np.ascontiguousarray(np.asarray(coef, dtype=np.float64).reshape(9))
    g, it = out_fld.grid, out_fld.internal
    check(_cabi.lib().dlesm_stencil9_step_dm(grid_mod.halo_plan(g), in_fld.device_ptr, out_fld.device_ptr,
                                             c.ctypes.data_as(C.POINTER(C.c_double)), g.nx, g.ny,
                                             it.xstart, it.xstop, it.ystart, it.ystop, _stream_ptr(stream)))


def invoke_continuity(ssha, sshn_t, sshn_u, sshn_v, hu, hv, un, vn, rdt, stream=None):
    """the continuity kernel (metadata: GO_GRID_AREA_T): fields on T, U and V points, the grid's cell
    area from the PSy layer (its device mirror), over ssha%internal"""
    g, it = ssha.grid, ssha.internal
    check(_cabi.lib().dlesm_continuity_f64(float(rdt), g.nx, g.ny, it.xstart, it.xstop, it.ystart, it.ystop,
                                           sshn_t.device_ptr, sshn_u.device_ptr, sshn_v.device_ptr, hu.device_ptr,
                                           hv.device_ptr, un.device_ptr, vn.device_ptr,
                                           C.c_void_p(g.area_t_device.data_ptr()), ssha.device_ptr, _stream_ptr(stream)))


def momentum_params(rdt, cbfr, visc, g):
    """constants of the momentum kernels: time step, bottom friction, viscosity, gravity"""
    return _cabi.MomentumParams(rdt=float(rdt), cbfr=float(cbfr), visc=float(visc), g=float(g))


def coriolis(grid, omega=7.292116e-5, d2r=math.pi / 180.0):
    """the Coriolis parameter of the momentum kernels, once per grid: fcor_u = (2*omega)*sin(gphiu*d2r) and fcor_v from
    gphiv, computed on the host with the host's sin and uploaded.  Returns (fcor_u, fcor_v), the
    device tensors; a second call with the same constants returns the cached pair."""
    import numpy as np
    import torch
    if grid.gphiu is None:
        raise _cabi.GoceanStop(_cabi.EABORT, "coriolis: grid%gphiu requested before grid_init")
    if grid.fcor is not None and grid.fcor[0] == omega and grid.fcor[1] == d2r:
        return grid.fcor[2], grid.fcor[3]
    fu, fv = ((2.0 * omega) * np.sin(gphi * d2r) for gphi in (grid.gphiu, grid.gphiv))
    fu, fv = torch.from_numpy(np.ascontiguousarray(fu)).cuda(), torch.from_numpy(np.ascontiguousarray(fv)).cuda()
    torch.cuda.current_stream().synchronize()              # in place before a kernel on another stream reads them
    grid.fcor = (omega, d2r, fu, fv)
    return fu, fv


def _momentum_grid(g, who):
    """the grid's device mirrors as a dlesm_momentum_grid; refuses a grid whose Coriolis parameter was never set"""
    if g.fcor is None:
        raise _cabi.GoceanStop(_cabi.EABORT, f"{who}: the Coriolis parameter of this grid has not been set: call "
                                             "psy.coriolis(grid) once before the momentum kernels")
    mg = _cabi.MomentumGrid()
    for name in _cabi.MOMENTUM_GRID_ARRAYS:
        t = g.fcor[2 if name == "fcor_u" else 3] if name.startswith("fcor") else getattr(g, name + "_device")
        setattr(mg, name, t.data_ptr())
    return mg


def invoke_momentum_u(params, ua, un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, stream=None):
    """momentum_u over ua%internal: ua where both T cells of the u face are wet"""
    g, it = ua.grid, ua.internal
    mg = _momentum_grid(g, "invoke_momentum_u")
    check(_cabi.lib().dlesm_momentum_u_f64(C.byref(params), C.byref(mg), g.nx, g.ny, it.xstart, it.xstop, it.ystart, it.ystop,
                                           *[f.device_ptr for f in (un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, ua)],
                                           _stream_ptr(stream)))


def invoke_momentum_v(params, va, un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_v, stream=None):
    """momentum_v over va%internal: va where both T cells of the v face are wet"""
    g, it = va.grid, va.internal
    mg = _momentum_grid(g, "invoke_momentum_v")
    check(_cabi.lib().dlesm_momentum_v_f64(C.byref(params), C.byref(mg), g.nx, g.ny, it.xstart, it.xstop, it.ystart, it.ystop,
                                           *[f.device_ptr for f in (un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_v, va)],
                                           _stream_ptr(stream)))


def invoke_momentum(params, ua, va, un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, ssha_v, stream=None):
    """both momentum loop nests in one sweep: momentum_u over ua%internal and momentum_v over va%internal, bit for bit
    invoke_momentum_u then invoke_momentum_v, at 180 instead of 2 x 140 B/cell"""
    g = ua.grid
    mg = _momentum_grid(g, "invoke_momentum")
    check(_cabi.lib().dlesm_momentum_f64(C.byref(params), C.byref(mg), g.nx, g.ny, C.byref(ua.internal), C.byref(va.internal),
                                         *[f.device_ptr for f in (un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, ssha_v,
                                                                  ua, va)],
                                         _stream_ptr(stream)))


def invoke_next_sshu(sshn_u, sshn_t, stream=None):
    """next_sshu over sshn_u%internal: the grid's tmask, area_t and area_u mirrors"""
    g, it = sshn_u.grid, sshn_u.internal
    check(_cabi.lib().dlesm_next_sshu_f64(g.nx, g.ny, it.xstart, it.xstop, it.ystart, it.ystop, g.tmask_device_ptr,
                                          C.c_void_p(g.area_t_device.data_ptr()), C.c_void_p(g.area_u_device.data_ptr()),
                                          sshn_t.device_ptr, sshn_u.device_ptr, _stream_ptr(stream)))


def invoke_next_sshv(sshn_v, sshn_t, stream=None):
    """next_sshv over sshn_v%internal: the grid's tmask, area_t and area_v mirrors"""
    g, it = sshn_v.grid, sshn_v.internal
    check(_cabi.lib().dlesm_next_sshv_f64(g.nx, g.ny, it.xstart, it.xstop, it.ystart, it.ystop, g.tmask_device_ptr,
                                          C.c_void_p(g.area_t_device.data_ptr()), C.c_void_p(g.area_v_device.data_ptr()),
                                          sshn_t.device_ptr, sshn_v.device_ptr, _stream_ptr(stream)))


class OpenBoundary:
    """the open-boundary plan of a grid (dlesm_obc): lists of the open T cells, u faces and v faces of
    the T-, U- and V-point internal regions, in HBM.  Made by open_boundary(grid); grid_init releases it."""

    def __init__(self, handle, nt, nu, nv):
        self.handle, self.nt, self.nu, self.nv = handle, nt, nu, nv

    def __repr__(self):
        return f"OpenBoundary(open T cells {self.nt}, u faces {self.nu}, v faces {self.nv})"


def open_boundary(grid):
    """the grid's open-boundary plan, built once per grid from its host tmask and the T/U/V internal regions (DESIGN.md
    section 6.6).  A mask the plan refuses (an open face whose inner face is open, or lies at the edge of the array) stops
    with GoceanStop."""
    if grid._obc is None:
        from .field_mod import GO_T_POINTS, GO_U_POINTS, GO_V_POINTS, field_bounds
        if grid.tmask is None:
            raise _cabi.GoceanStop(_cabi.EABORT, "open_boundary: grid%tmask requested before grid_init")
        import numpy as np
        tm = np.ascontiguousarray(grid.tmask, dtype=np.int32)
        boxes = [field_bounds(grid, p)[0] for p in (GO_T_POINTS, GO_U_POINTS, GO_V_POINTS)]
        h = C.c_void_p()
        rc = _cabi.lib().dlesm_obc_create(tm.ctypes.data, grid.nx, grid.ny, *[C.byref(b) for b in boxes], C.byref(h))
        if rc != 0:
            raise _cabi.GoceanStop(_cabi.EABORT, "open_boundary: " + _cabi.lib().dlesm_last_error().decode())
        n = [C.c_int() for _ in range(3)]
        check(_cabi.lib().dlesm_obc_counts(h, *[C.byref(x) for x in n]))
        grid._obc = OpenBoundary(h, *[x.value for x in n])
    return grid._obc


class WetPlan:
    """the wet plan of a grid (dlesm_wet_plan): which wave tiles of the one-sweep step over the T
    internal region store anything but land ssha.  Made by wet_plan(grid); grid_init releases it."""

    def __init__(self, handle, tiles, active):
        self.handle, self.tiles, self.active = handle, tiles, active

    def __repr__(self):
        return f"WetPlan(tiles {self.tiles}, active {self.active})"


def wet_plan(grid):
    """the grid's wet plan, built once per grid from its host tmask (the mask its device mirror holds) and the T internal
    region"""
    if grid._wet is None:
        from .field_mod import GO_T_POINTS, field_bounds
        if grid.tmask is None:
            raise _cabi.GoceanStop(_cabi.EABORT, "wet_plan: grid%tmask requested before grid_init")
        import numpy as np
        tm = np.ascontiguousarray(grid.tmask, dtype=np.int32)
        box = field_bounds(grid, GO_T_POINTS)[0]
        h = C.c_void_p()
        rc = _cabi.lib().dlesm_wet_plan_create(tm.ctypes.data, grid.nx, grid.ny, C.byref(box), C.byref(h))
        if rc != 0:
            raise _cabi.GoceanStop(_cabi.EABORT, "wet_plan: " + _cabi.lib().dlesm_last_error().decode())
        n = [C.c_longlong() for _ in range(2)]
        check(_cabi.lib().dlesm_wet_plan_counts(h, *[C.byref(x) for x in n]))
        grid._wet = WetPlan(h, *[x.value for x in n])
    return grid._wet


def tide_ssh(amp, omega, t):
    """the boundary sea-surface height of bc_ssh, amp*sin(omega*t), with the host's sin"""
    return float(amp) * math.sin(float(omega) * float(t))


def invoke_bc_ssh(ssha, ssh_bc, stream=None):
    """bc_ssh: ssha = ssh_bc on the open T cells of ssha%internal"""
    check(_cabi.lib().dlesm_bc_ssh_f64(open_boundary(ssha.grid).handle, float(ssh_bc), ssha.device_ptr, _stream_ptr(stream)))


def invoke_bc_flather_u(params, ua, hu, sshn_u, sshn_t, stream=None):
    """Flather on the open u faces of ua%internal, ua in place"""
    check(_cabi.lib().dlesm_bc_flather_u_f64(open_boundary(ua.grid).handle, C.byref(params), hu.device_ptr, sshn_u.device_ptr,
                                             sshn_t.device_ptr, ua.device_ptr, _stream_ptr(stream)))


def invoke_bc_flather_v(params, va, hv, sshn_v, sshn_t, stream=None):
    """Flather on the open v faces of va%internal, va in place"""
    check(_cabi.lib().dlesm_bc_flather_v_f64(open_boundary(va.grid).handle, C.byref(params), hv.device_ptr, sshn_v.device_ptr,
                                             sshn_t.device_ptr, va.device_ptr, _stream_ptr(stream)))


def invoke_bc_open(params, ssh_bc, ssha, ua, va, hu, sshn_u, hv, sshn_v, sshn_t, stream=None):
    """bc_ssh, Flather on u and Flather on v in one launch, bit for bit the three separate calls"""
    check(_cabi.lib().dlesm_bc_open_f64(open_boundary(ssha.grid).handle, C.byref(params), float(ssh_bc),
                                        *[f.device_ptr for f in (hu, sshn_u, hv, sshn_v, sshn_t, ssha, ua, va)],
                                        _stream_ptr(stream)))


def invoke_nemolite_step(params, ssha, ssha_u, ssha_v, ua, va, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, ssh_bc=None,
                         stream=None, skip_land=False):
    """one NEMOLite2D-class time step in one call, bit for bit invoke_continuity (rdt = params.rdt)
    -> invoke_next_sshu / invoke_next_sshv on ssha -> invoke_momentum -> invoke_bc_open on the grid's open_boundary plan.
    ssh_bc=None: a closed basin, no boundary pass.  ssha is in/out (the ring cells east and north of the box are read).
    Single domain: stops on a decomposed grid, and when the grid's Coriolis parameter was never set.
    skip_land=True: the sweep leaves out the wave tiles of the grid's wet_plan that hold nothing but land (DESIGN.md section
    6.9) -- ssha_u, ssha_v, ua and va as without it in every cell, ssha in every cell with tmask != 0; a land cell of ssha
    may keep its content."""
    g = ssha.grid
    if g.decomp is not None and g.decomp.ndomains > 1:
        raise _cabi.GoceanStop(_cabi.EABORT, "invoke_nemolite_step: the grid is decomposed (%d subdomains): the step needs an "
                                             "ssha halo exchange between continuity and next_ssh*, which one call cannot "
                                             "hold; use the separate wrappers" % g.decomp.ndomains)
    mg = _momentum_grid(g, "invoke_nemolite_step")
    plan = None if ssh_bc is None else open_boundary(g).handle
    args = (C.byref(params), C.byref(mg), C.c_void_p(g.area_t_device.data_ptr()), g.nx, g.ny, C.byref(ssha.internal),
            C.byref(ua.internal), C.byref(va.internal), plan, 0.0 if ssh_bc is None else float(ssh_bc),
            *[f.device_ptr for f in (un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, ssha, ssha_u, ssha_v, ua, va)],
            _stream_ptr(stream))
    if skip_land:
        check(_cabi.lib().dlesm_nemolite_step_wet_f64(wet_plan(g).handle, *args))
    else:
        check(_cabi.lib().dlesm_nemolite_step_f64(*args))


def invoke_nemolite_step_dm(params, ssha, ssha_u, ssha_v, ua, va, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, ssh_bc=None,
                            stream=None, skip_land=False):
    """one NEMOLite2D-class time step and ONE exchange of its five outputs on a decomposed grid, bit for
    bit invoke_continuity -> ssha.halo_exchange(1) -> invoke_next_sshu / invoke_next_sshv -> invoke_momentum ->
    invoke_bc_open on this rank's open_boundary plan (ssh_bc=None: none) -> halo_exchange_multi of ssha, ssha_u, ssha_v, ua,
    va.  The inputs need valid depth-1 halos, corners included; the outputs leave with them.  Collective.  Stops on a grid
    with halo_width other than 1, and when the grid's Coriolis parameter was never set.  skip_land=True: as
    invoke_nemolite_step, with this rank's wet_plan (dlesm_nemolite_step_wet_dm)."""
    g = ssha.grid
    hw = getattr(g, "halo_width", 1)
    if hw != 1:
        raise _cabi.GoceanStop(_cabi.EABORT, "invoke_nemolite_step_dm: the grid has halo_width %d; the step exchanges depth-1 "
                                             "halos: decompose the grid with halo_width = 1" % hw)
    mg = _momentum_grid(g, "invoke_nemolite_step_dm")
    if getattr(g, "comm_tables", None) is None:
        raise _cabi.DlesmError(_cabi.EINVAL, "invoke_nemolite_step_dm: the grid has no message tables (grid_init after "
                                             "decompose)")
    obc = None if ssh_bc is None else open_boundary(g).handle
    args = (C.byref(params), C.byref(mg), C.c_void_p(g.area_t_device.data_ptr()), g.nx, g.ny, C.byref(ssha.internal),
            C.byref(ua.internal), C.byref(va.internal), obc, 0.0 if ssh_bc is None else float(ssh_bc),
            *[f.device_ptr for f in (un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, ssha, ssha_u, ssha_v, ua, va)],
            _stream_ptr(stream))
    if skip_land:
        check(_cabi.lib().dlesm_nemolite_step_wet_dm(grid_mod.halo_plan(g), wet_plan(g).handle, *args))
    else:
        check(_cabi.lib().dlesm_nemolite_step_dm(grid_mod.halo_plan(g), *args))


def _tracer_ptrs(who, c_out, c_in):
    """the pointer arrays of the tracers, c_in's and c_out's, and their number"""
    c_out, c_in = list(c_out), list(c_in)
    if len(c_out) != len(c_in):
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: %d output fields for %d tracers" % (who, len(c_out), len(c_in)))
    n = len(c_in)
    return (C.c_void_p * max(n, 1))(*[f.device_ptr for f in c_in]), (C.c_void_p * max(n, 1))(*[f.device_ptr for f in c_out]), n


def _tracer_args(who, rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, stream):
    pin, pout, n = _tracer_ptrs(who, c_out, c_in)
    g, it = ssha.grid, ssha.internal
    return (float(rdt), g.nx, g.ny, it.xstart, it.xstop, it.ystart, it.ystop, g.tmask_device_ptr,
            C.c_void_p(g.area_t_device.data_ptr()), *[f.device_ptr for f in (un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, ssha)],
            pin, pout, n, _stream_ptr(stream))


_TRACER_HALO_STOP = {1: "%s: the grid has halo_width %d; the step exchanges depth-1 halos: decompose the grid with halo_width = 1",
                     2: "%s: the grid has halo_width %d; the step reads two cells and exchanges depth-2 halos: decompose the "
                        "grid with halo_width = 2"}


def _tracer_step(who, entry, halo_width, rdt, c_out, c_in, ssha, *flow, stream=None):
    """the body of the six invoke_tracer_step* wrappers: `who` in front of every stop, the C entry `entry`, and the halo width
    a decomposed grid must have (None: the single-domain wrapper, which stops on a decomposed grid)"""
    g = ssha.grid
    if halo_width is None:
        if g.decomp is not None and g.decomp.ndomains > 1:
            raise _cabi.GoceanStop(_cabi.EABORT, "%s: the grid is decomposed (%d subdomains): the new tracers need a halo "
                                                 "exchange; use %s_dm" % (who, g.decomp.ndomains, who))
        plan = ()
    else:
        hw = getattr(g, "halo_width", 1)
        if hw != halo_width:
            raise _cabi.GoceanStop(_cabi.EABORT, _TRACER_HALO_STOP[halo_width] % (who, hw))
        if getattr(g, "comm_tables", None) is None:
            raise _cabi.DlesmError(_cabi.EINVAL, "%s: the grid has no message tables (grid_init after decompose)" % who)
        plan = (grid_mod.halo_plan(g),)
    check(getattr(_cabi.lib(), entry)(*plan, *_tracer_args(who, rdt, c_out, c_in, ssha, *flow, stream)))


def invoke_tracer_step(rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, stream=None):
    """upwind transport of up to TRACER_MAX T-point tracers in one sweep: c_out[k] <- c_in[k] carried by
    continuity's face transports of level n (un, vn, hu, hv, sshn_u, sshn_v), from the water column ht + sshn_t to ht + ssha,
    over the T internal region, on wet cells only.  c_out and c_in are lists of T-point fields; ssha is what the time step
    made from the same level-n inputs.  Single domain: stops on a decomposed grid."""
    _tracer_step("invoke_tracer_step", "dlesm_tracer_step_f64", None, rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, sshn_t, sshn_u,
                 sshn_v, stream=stream)


def invoke_tracer_step_dm(rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, stream=None):
    """invoke_tracer_step and ONE exchange of the new tracers on a decomposed grid (dlesm_tracer_step_dm, DESIGN.md section
    6.10), bit for bit invoke_tracer_step -> halo_exchange_multi(c_out).  The flow fields and c_in need valid depth-1 halos;
    c_out leaves with them.  Collective.  Stops on a grid with halo_width other than 1."""
    _tracer_step("invoke_tracer_step_dm", "dlesm_tracer_step_dm", 1, rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, sshn_t, sshn_u,
                 sshn_v, stream=stream)


def invoke_tracer_step_muscl(rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, stream=None):
    """invoke_tracer_step with second-order limited face values (dlesm_tracer_step_muscl_f64): the
    upwind cell's monotonised-central slope rebuilds what a face carries; land, open cells and cells next to land keep the
    upwind value.  Same arguments and rules.  Single domain: stops on a decomposed grid."""
    _tracer_step("invoke_tracer_step_muscl", "dlesm_tracer_step_muscl_f64", None, rdt, c_out, c_in, ssha, un, vn, ht, hu, hv,
                 sshn_t, sshn_u, sshn_v, stream=stream)


def invoke_tracer_step_muscl_dm(rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, stream=None):
    """invoke_tracer_step_muscl and ONE depth-2 exchange of the new tracers on a decomposed grid (dlesm_tracer_step_muscl_dm,
    DESIGN.md section 6.11), bit for bit invoke_tracer_step_muscl -> halo_exchange_multi(c_out).  The grid's mask and c_in
    need valid depth-2 halos, the flow fields depth-1 halos; c_out leaves with depth-2 halos.  Collective.  Stops on a grid
    with halo_width other than 2."""
    _tracer_step("invoke_tracer_step_muscl_dm", "dlesm_tracer_step_muscl_dm", 2, rdt, c_out, c_in, ssha, un, vn, ht, hu, hv,
                 sshn_t, sshn_u, sshn_v, stream=stream)


def invoke_tracer_step_hancock(rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, stream=None):
    """invoke_tracer_step_muscl with time-centred face values (dlesm_tracer_step_hancock_f64): the
    slope's factor 0.5 becomes 0.5 * (1 - n), n the face's Courant number in its upwind cell, 0 where n is not in [0, 1).
    Same arguments and rules.  Single domain: stops on a decomposed grid."""
    _tracer_step("invoke_tracer_step_hancock", "dlesm_tracer_step_hancock_f64", None, rdt, c_out, c_in, ssha, un, vn, ht, hu,
                 hv, sshn_t, sshn_u, sshn_v, stream=stream)


def invoke_tracer_step_hancock_dm(rdt, c_out, c_in, ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, stream=None):
    """invoke_tracer_step_hancock and ONE depth-2 exchange of the new tracers on a decomposed grid
    (dlesm_tracer_step_hancock_dm), bit for bit invoke_tracer_step_hancock ->
    halo_exchange_multi(c_out).  The grid's mask and c_in need valid depth-2 halos, the flow fields depth-1 halos (area_t, ht
    and sshn_t among them: w of the cell beyond the box is built from them); c_out leaves with depth-2 halos.  Collective.
    Stops on a grid with halo_width other than 2."""
    _tracer_step("invoke_tracer_step_hancock_dm", "dlesm_tracer_step_hancock_dm", 2, rdt, c_out, c_in, ssha, un, vn, ht, hu, hv,
                 sshn_t, sshn_u, sshn_v, stream=stream)


TracerCourantResult = collections.namedtuple(
    "TracerCourantResult", "face_max outflow_max face_at outflow_at face_over outflow_over invalid wet rdt_limit")


def tracer_courant(rdt, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, face_limit=0.5, outflow_limit=1.0, stream=None):
    """"may I take a tracer step with this rdt" (dlesm_tracer_courant_async_f64): one read-only sweep
    over the level-n flow, over the T internal region with the grid's mask and area_t, that needs no ssha -- callable before
    the flow step.  Returns a TracerCourantResult, the same on every rank:
      face_max      the largest face Courant number of a wet cell, exactly as invoke_tracer_step_hancock computes it (the
                    limited sweeps keep a profile's range while it is <= 1/2; the Hancock sweep falls back to the upwind face
                    value where it is >= 1);
      outflow_max   the largest outflow number of a wet cell (the upwind sweep keeps c >= 0 while it is <= 1);
      face_at, outflow_at   (rank, i, j) of a cell that attains each: the lowest rank (1-based, parallel_mod.get_rank) that
                    holds one and the local 1-based indices of its first such cell, or None;
      face_over, outflow_over   wet cells with a face number >= face_limit / an outflow number >= outflow_limit;
      invalid       wet cells in which a number is not finite and >= 0 (they enter no maximum);  wet: the wet cells;
      rdt_limit     rdt * min(face_limit / face_max, outflow_limit / outflow_max), inf when both maxima are 0 -- an
                    ESTIMATE of the largest rdt that keeps both limits: the numbers are linear in rdt only up to rounding.
    On a decomposed grid the flow fields need valid depth-1 halos; collective there."""
    g, it = sshn_t.grid, sshn_t.internal
    r = _cabi.TracerCourant.from_buffer_copy(_fetch_record(               # (see there for where the record lives)
        stream, sshn_t.data.device, 8, lambda res, s: check(_cabi.lib().dlesm_tracer_courant_async_f64(
            float(rdt), g.nx, g.ny, it.xstart, it.xstop, it.ystart, it.ystop, g.tmask_device_ptr,
            C.c_void_p(g.area_t_device.data_ptr()), *[f.device_ptr for f in (un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v)],
            float(face_limit), float(outflow_limit), res, s))))
    face_max, face_at = parallel_mod._place(r.face_max, r.face_index, g.nx)
    outflow_max, outflow_at = parallel_mod._place(r.outflow_max, r.outflow_index, g.nx)
    counts = [parallel_mod._global_count(c) for c in (r.face_over, r.outflow_over, r.invalid, r.wet)]
    ratio = min(float(face_limit) / face_max if face_max > 0.0 else math.inf,
                float(outflow_limit) / outflow_max if outflow_max > 0.0 else math.inf)
    return TracerCourantResult(face_max, outflow_max, face_at, outflow_at, *counts,
                               float(rdt) * ratio if ratio != math.inf else math.inf)


def tracer_courant_check(rdt, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, face_limit=0.5, outflow_limit=1.0, stream=None):
    """tracer_courant, and DlesmError -- on every rank -- when a wet cell holds a number that is not finite and >= 0, reaches
    face_limit or reaches outflow_limit.  The message names which of the three, the value, and the rank and local 1-based
    (i, j) of the cell that holds the maximum (an invalid cell enters no maximum: its count is all the record has).  Returns
    the TracerCourantResult otherwise."""
    r = tracer_courant(rdt, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, face_limit, outflow_limit, stream)
    if r.invalid > 0:
        why = "invalid: %d wet cell(s) hold a Courant number that is not finite and >= 0 (rdt = %r)" % (r.invalid, float(rdt))
    elif r.face_over > 0:
        why = "face_over: %d wet cell(s) reach face_limit = %r; face_max = %r %s" % (
            r.face_over, float(face_limit), r.face_max, parallel_mod._where(r.face_at))
    elif r.outflow_over > 0:
        why = "outflow_over: %d wet cell(s) reach outflow_limit = %r; outflow_max = %r %s" % (
            r.outflow_over, float(outflow_limit), r.outflow_max, parallel_mod._where(r.outflow_at))
    else:
        return r
    raise _cabi.DlesmError(_cabi.EABORT, "tracer_courant_check: %s; rdt_limit = %r" % (why, r.rdt_limit))


FlowCourantResult = collections.namedtuple(
    "FlowCourantResult", "gravity_max advective_max viscous_max depth_min gravity_at advective_at viscous_at depth_at "
    "gravity_over advective_over viscous_over shallow invalid wet rdt_limit")


def _flow_constants(who, g, visc, params):
    """g and visc where the momentum wrappers take theirs: the caller's momentum_params, unless given by keyword"""
    if g is None and params is not None:
        g = params.g
    if visc is None and params is not None:
        visc = params.visc
    if g is None or visc is None:
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: g and visc, or params = psy.momentum_params(...)" % who)
    return float(g), float(visc)


def flow_courant(rdt, un, vn, ht, sshn_t, g=None, visc=None, gravity_limit=1.0, advective_limit=1.0, viscous_limit=0.25,
                 depth_limit=0.0, params=None, stream=None):
    """"may the flow step take this rdt" (dlesm_flow_courant_async_f64): one read-only sweep over the
    level-n flow, over the T internal region with the grid's mask, dx_t and dy_t.  g and visc default to those of `params`, the
    momentum_params the flow step is called with.  Returns a FlowCourantResult, the same on every rank:
      gravity_max   the largest gravity-wave number rdt * sqrt(g d) * sqrt(1/dx^2 + 1/dy^2) of a wet cell, d = ht + sshn_t;
      advective_max the largest advective number rdt * (max|u| / dx + max|v| / dy) over a cell's faces that do not touch land;
      viscous_max   the largest viscous number rdt * visc * (1/dx^2 + 1/dy^2);  depth_min: the smallest water column d;
      gravity_at .. depth_at   (rank, i, j) of a cell that attains each: the lowest rank (1-based, parallel_mod.get_rank) that
                    holds one and the local 1-based indices of its first such cell, or None;
      gravity_over, advective_over, viscous_over   wet cells with the number >= its limit;  shallow: with d <= depth_limit;
      invalid       wet cells with a column that is not finite and > 0 or a number that is not finite and >= 0 (they enter
                    nothing else);  wet: the wet cells;
      rdt_limit     rdt * min(limit / maximum) over the three maxima that are not 0, inf when all are -- an ESTIMATE of the
                    largest rdt that keeps the three limits: the numbers are linear in rdt only up to rounding.
    On a decomposed grid the fields need valid depth-1 halos; collective there."""
    gv, nu = _flow_constants("flow_courant", g, visc, params)
    grid, it = sshn_t.grid, sshn_t.internal
    limits = (float(gravity_limit), float(advective_limit), float(viscous_limit))
    r = _cabi.FlowCourant.from_buffer_copy(_fetch_record(                 # (see there for where the record lives)
        stream, sshn_t.data.device, 16, lambda res, s: check(_cabi.lib().dlesm_flow_courant_async_f64(
            float(rdt), gv, nu, grid.nx, grid.ny, it.xstart, it.xstop, it.ystart, it.ystop, grid.tmask_device_ptr,
            C.c_void_p(grid.dx_t_device.data_ptr()), C.c_void_p(grid.dy_t_device.data_ptr()),
            *[f.device_ptr for f in (un, vn, ht, sshn_t)], *limits, float(depth_limit), res, s))))
    tops, ats = [], []
    for top, index in ((r.gravity_max, r.gravity_index), (r.advective_max, r.advective_index),
                       (r.viscous_max, r.viscous_index), (-r.depth_min, r.depth_index)):   # the minimum as a maximum of -d
        top, at = parallel_mod._place(top, index, grid.nx)
        tops.append(top), ats.append(at)
    tops[3] = -tops[3]
    counts = [parallel_mod._global_count(c)
              for c in (r.gravity_over, r.advective_over, r.viscous_over, r.shallow, r.invalid, r.wet)]
    ratio = min(lim / top if top > 0.0 else math.inf for lim, top in zip(limits, tops[:3]))
    return FlowCourantResult(*tops, *ats, *counts, float(rdt) * ratio if ratio != math.inf else math.inf)


def flow_courant_check(rdt, un, vn, ht, sshn_t, g=None, visc=None, gravity_limit=1.0, advective_limit=1.0,
                       viscous_limit=0.25, depth_limit=0.0, params=None, stream=None):
    """flow_courant, and DlesmError -- on every rank -- when a wet cell is invalid, reaches one of the three limits or is no
    deeper than depth_limit.  The message names which, the value, and the rank and local 1-based (i, j) of the cell that
    holds the extreme (an invalid cell enters no extreme: its count is all the record has).  Returns the FlowCourantResult
    otherwise."""
    r = flow_courant(rdt, un, vn, ht, sshn_t, g, visc, gravity_limit, advective_limit, viscous_limit, depth_limit, params,
                     stream)
    if r.invalid > 0:
        why = "invalid: %d wet cell(s) hold a water column that is not finite and > 0 or a number that is not finite and " \
              ">= 0 (rdt = %r)" % (r.invalid, float(rdt))
    elif r.gravity_over > 0:
        why = "gravity_over: %d wet cell(s) reach gravity_limit = %r; gravity_max = %r %s" % (
            r.gravity_over, float(gravity_limit), r.gravity_max, parallel_mod._where(r.gravity_at))
    elif r.advective_over > 0:
        why = "advective_over: %d wet cell(s) reach advective_limit = %r; advective_max = %r %s" % (
            r.advective_over, float(advective_limit), r.advective_max, parallel_mod._where(r.advective_at))
    elif r.viscous_over > 0:
        why = "viscous_over: %d wet cell(s) reach viscous_limit = %r; viscous_max = %r %s" % (
            r.viscous_over, float(viscous_limit), r.viscous_max, parallel_mod._where(r.viscous_at))
    elif r.shallow > 0:
        why = "shallow: %d wet cell(s) are no deeper than depth_limit = %r; depth_min = %r %s" % (
            r.shallow, float(depth_limit), r.depth_min, parallel_mod._where(r.depth_at))
    else:
        return r
    raise _cabi.DlesmError(_cabi.EABORT, "flow_courant_check: %s; rdt_limit = %r" % (why, r.rdt_limit))


def step_rdt_limit(rdt, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, g=None, visc=None, gravity_limit=1.0, advective_limit=1.0,
                   viscous_limit=0.25, face_limit=0.5, outflow_limit=1.0, params=None, stream=None):
    """the one call an adaptive time loop needs: flow_courant and tracer_courant on the same level-n fields, and the smaller
    of their two rdt_limit estimates (inf when the flow is at rest on a grid without gravity waves to resolve: never, in
    practice).  Nothing is raised for a limit that `rdt` itself passes; collective on a decomposed grid."""
    flow = flow_courant(rdt, un, vn, ht, sshn_t, g, visc, gravity_limit, advective_limit, viscous_limit, 0.0, params, stream)
    tracer = tracer_courant(rdt, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, face_limit, outflow_limit, stream)
    return min(flow.rdt_limit, tracer.rdt_limit)


def flow_output(un, vn, ht, sshn_t, ssh=None, ut=None, vt=None, speed=None, ke=None, vort=None, weight=None, stream=None):
    """the model's output fields in one sweep (dlesm_flow_output_f64): of the level-n flow, into the
    T-point fields given -- ssh (sshn_t itself), ut and vt (the velocities brought to the T point, a face on land carrying
    nothing), speed (their modulus), ke (0.5 * (ht + sshn_t) * (ut^2 + vt^2)) and vort (dv/dx - du/dy at the cell's NE corner,
    stored only where the cells east, north and north-east are not land).  weight = None stores the values; a number adds
    weight * value to what the fields hold (a time mean over nsteps: weight = 1 / nsteps into zeroed fields).  Over the T
    internal region with the grid's mask, dx_v and dy_u; land and open cells and every halo keep their content.  ht may be
    None unless ke is wanted, sshn_t unless ssh or ke is.  On a decomposed grid un, vn and the mask need valid depth-1 halos,
    corners included (grid_mod.exchange_mask_halos fills the mask's); nothing is exchanged and the call is not collective."""
    who = "flow_output"
    outs = (ssh, ut, vt, speed, ke, vort)
    first = next((f for f in outs if f is not None), None)
    if first is None:
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: no output field" % who)
    g, it = first.grid, first.internal
    for f in outs:
        if f is not None and (f.grid is not g or f.defined_on != GO_T_POINTS):
            raise _cabi.DlesmError(_cabi.EINVAL, "%s: the outputs are T-point fields of one grid" % who)
    if un.grid is not g or vn.grid is not g:
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: un, vn and the outputs are fields of one grid" % who)
    pout = (C.c_void_p * _cabi.OUT_COUNT)(*[f.device_ptr if f is not None else None for f in outs])
    need_st, need_ht = ssh is not None or ke is not None, ke is not None
    if (need_st and sshn_t is None) or (need_ht and ht is None):
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: ke needs ht and sshn_t, ssh needs sshn_t" % who)
    metric = vort is not None
    check(_cabi.lib().dlesm_flow_output_f64(
        _cabi.OUT_SET if weight is None else _cabi.OUT_ADD, 0.0 if weight is None else float(weight), g.nx, g.ny, it.xstart,
        it.xstop, it.ystart, it.ystop, g.tmask_device_ptr,
        C.c_void_p(g.dx_v_device.data_ptr()) if metric else None, C.c_void_p(g.dy_u_device.data_ptr()) if metric else None,
        un.device_ptr, vn.device_ptr, ht.device_ptr if need_ht else None, sshn_t.device_ptr if need_st else None, pout,
        _stream_ptr(stream)))


def _drifter_arrays(who, px, py, status):
    import torch
    if not (px.is_cuda and py.is_cuda and status.is_cuda and px.is_contiguous() and py.is_contiguous() and
            status.is_contiguous()):
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: px, py and status are contiguous CUDA tensors" % who)
    if px.dtype != torch.float64 or py.dtype != torch.float64 or status.dtype != torch.int32:
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: px and py are float64, status is int32" % who)
    n = px.numel()
    if py.numel() != n or status.numel() != n:
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: px, py and status hold one element per particle" % who)
    return n


def _particle_step(who, entry, h, nsub, px, py, status, un, vn, own=None, rng=None, stream=None):
    """what drifter_step, dispersal_step and random_walk share: the checks of the arrays and of the one grid, the T internal
    box and the call of `entry`.  own(g): the entry's own argument behind nsub (kh, or kh_t's address), made where the entry
    looks at it; rng = (seed, tick, ids, tick_dev) for the two entries that draw numbers."""
    import torch

    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    n = _drifter_arrays(who, px, py, status)
    g = un.grid
    if vn.grid is not g:
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: un and vn are fields of one grid" % who)
    head, id_arg = [float(h), int(nsub)] + ([own(g)] if own is not None else []), []
    if rng is not None:
        seed, tick, ids, tick_dev = rng
        if ids is not None and not (ids.is_cuda and ids.is_contiguous() and ids.dtype == torch.int32 and ids.numel() == n):
            raise _cabi.DlesmError(_cabi.EINVAL, "%s: ids is a contiguous int32 CUDA tensor of one element per particle" % who)
        if tick_dev is not None and not (tick_dev.is_cuda and tick_dev.dtype == torch.int64 and tick_dev.numel() == 1):
            raise _cabi.DlesmError(_cabi.EINVAL, "%s: tick_dev is a one-element int64 CUDA tensor" % who)
        seed = int(seed) & 0xffffffffffffffff
        head += [seed - (1 << 64) if seed >> 63 else seed, int(tick), ptr(tick_dev)]
        id_arg = [ptr(ids)]
    it = field_bounds(g, GO_T_POINTS)[0]
    check(entry(*head, g.nx, g.ny, it.xstart, it.xstop, it.ystart, it.ystop, g.tmask_device_ptr, ptr(g.dx_t_device),
                ptr(g.dy_t_device), un.device_ptr, vn.device_ptr, n, *id_arg, ptr(px), ptr(py), ptr(status), _stream_ptr(stream)))


def drifter_step(h, px, py, status, un, vn, nsub=1, stream=None):
    """carry particles through the level-n C-grid flow (dlesm_drifter_step_f64): nsub substeps of h
    seconds by the midpoint rule, in place.  px, py: contiguous float64 CUDA tensors, positions in local index coordinates (T
    cell (i, j), 1-based, covers [i, i+1) x [j, j+1)); status: a contiguous int32 CUDA tensor of _cabi.DRIFTER_* numbers, only
    DRIFTER_ACTIVE particles are read or written.  A particle that leaves the T internal region becomes DRIFTER_LEFT and one
    that reaches an open cell DRIFTER_OPEN, both at their new position; one whose move would end on land becomes
    DRIFTER_GROUNDED at its last wet position.  Over the T internal region of un.grid with the grid's tmask, dx_t and dy_t.
    Asynchronous.  On a decomposed grid un, vn and the mask need valid depth-1 halos; nothing is exchanged and the call is
    not collective."""
    _particle_step("drifter_step", _cabi.lib().dlesm_drifter_step_f64, h, nsub, px, py, status, un, vn, stream=stream)


def dispersal_step(h, kh, seed, tick, px, py, status, un, vn, nsub=1, ids=None, tick_dev=None, stream=None):
    """drifter_step with random-walk diffusion (dlesm_dispersal_step_f64): every substep adds a kick,
    uniform with variance 2 kh |h| per axis (kh: a constant horizontal diffusivity in m2/s), drawn from Philox4x32-10 with
    the seed as key and (particle id, tick + substep) as counter; a kick that would end on land is rejected.  In place; px, py,
    status, the grid, the box, the mask and the metrics as drifter_step.  seed: any 64 bits; tick: the substeps taken so far
    (>= 0) -- the caller advances it by nsub from call to call.  ids: None (the slot number is the identity) or a contiguous
    int32 CUDA tensor of one identity per particle, to be carried along when the particles are sorted.  tick_dev: None, or a
    one-element int64 CUDA tensor that the kernel adds to tick and the call advances by nsub on the stream: what a captured
    time loop needs, for a graph without it replays the same kicks.  Same seed, ids and ticks give the same bytes on any
    stream and any run.  Asynchronous; nothing is exchanged and the call is not collective."""
    _particle_step("dispersal_step", _cabi.lib().dlesm_dispersal_step_f64, h, nsub, px, py, status, un, vn, lambda g: float(kh),
                   (seed, tick, ids, tick_dev), stream)


def random_walk(h, kh_t, seed, tick, px, py, status, un, vn, nsub=1, ids=None, tick_dev=None, stream=None):
    """dispersal_step in a diffusivity that varies in space (dlesm_random_walk_f64).  kh_t: an
    r2d_field at T points of un's grid, or a contiguous float64 CUDA tensor of ny x nx laid out like the grid's dx_t, in
    m2/s; it must be finite and >= 0 wherever the mask is not 0 (what it holds on land changes no bit).  Per substep and axis
    a particle drifts by |h| dK/dx -- Visser's correction, without which particles collect where mixing is weak -- and takes
    a kick sized by K half a drift ahead, K linear between the cell's faces; a constant kh_t gives dispersal_step's bits.
    Everything else -- seed, tick, ids, tick_dev, the rejection at the coast, the statuses, the region -- is dispersal_step's.
    Keep |h| |dK| / dx^2 + sqrt(6 K |h|) / dx below one cell.  Asynchronous.  On a decomposed grid kh_t needs valid depth-1
    halos, like un, vn and the mask; nothing is exchanged and the call is not collective."""
    import torch
    who = "random_walk"

    def own(g):
        if isinstance(kh_t, torch.Tensor):
            if not (kh_t.is_cuda and kh_t.is_contiguous() and kh_t.dtype == torch.float64 and tuple(kh_t.shape) == (g.ny, g.nx)):
                raise _cabi.DlesmError(_cabi.EINVAL, "%s: kh_t is a contiguous float64 CUDA tensor of %d x %d" % (who, g.ny, g.nx))
            return C.c_void_p(kh_t.data_ptr())
        if kh_t.grid is not g or kh_t.defined_on != GO_T_POINTS:
            raise _cabi.DlesmError(_cabi.EINVAL, "%s: kh_t is a T-point field of the grid of un" % who)
        return kh_t.device_ptr

    _particle_step(who, _cabi.lib().dlesm_random_walk_f64, h, nsub, px, py, status, un, vn, own, (seed, tick, ids, tick_dev), stream)


def drifter_sample(px, py, status, fields, out=None, stream=None):
    """T-point fields at the particles (dlesm_drifter_sample_f64): for every DRIFTER_ACTIVE particle
    inside the T internal region, out[k][p] = fields[k] in the particle's cell, for 1 to 8 T-point r2d_fields of one grid;
    every other out[k][p] keeps its content.  out: a list of contiguous float64 CUDA tensors of one element per particle, or
    None for new ones filled with NaN.  Returns the list.  Asynchronous; nothing is exchanged."""
    import torch
    who = "drifter_sample"
    n = _drifter_arrays(who, px, py, status)
    fields = list(fields)
    if not 1 <= len(fields) <= _cabi.DRIFTER_MAX_FIELDS:
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: 1 to %d fields" % (who, _cabi.DRIFTER_MAX_FIELDS))
    g = fields[0].grid
    if any(f.grid is not g or f.defined_on != GO_T_POINTS for f in fields):
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: the fields are T-point fields of one grid" % who)
    if out is None:
        s = stream if stream is not None else torch.cuda.current_stream()
        with torch.cuda.stream(s):
            out = [torch.full((n,), float("nan"), dtype=torch.float64, device=px.device) for _ in fields]
    out = list(out)
    if len(out) != len(fields) or any(not (o.is_cuda and o.is_contiguous() and o.dtype == torch.float64 and o.numel() == n)
                                      for o in out):
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: out holds one contiguous float64 CUDA tensor of n elements per field" % who)
    it = fields[0].internal
    pf = (C.c_void_p * len(fields))(*[f.device_ptr for f in fields])
    po = (C.c_void_p * len(fields))(*[o.data_ptr() for o in out])
    check(_cabi.lib().dlesm_drifter_sample_f64(
        g.nx, g.ny, it.xstart, it.xstop, it.ystart, it.ystop, n, C.c_void_p(px.data_ptr()), C.c_void_p(py.data_ptr()),
        C.c_void_p(status.data_ptr()), pf, po, len(fields), _stream_ptr(stream)))
    return out


def _on(stream):
    import torch
    return torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream())


def particle_order(px, py, status, grid, perm=None, stream=None):
    """the particles' cell order (dlesm_particle_order_f64): perm, a contiguous int32 CUDA tensor of
    one element per particle (made when None), becomes the stable ascending order of the keys
    (floor(py) - ystart) * nxb + (floor(px) - xstart) of the DRIFTER_ACTIVE particles inside the T internal region of `grid`
    -- the box drifter_step uses -- with every other particle behind them in its old order.  Returns (perm, nlive), nlive a
    one-element int32 CUDA tensor: the number of particles in front.  Asynchronous, no synchronisation; the scratch is a
    tensor of the caching allocator made on `stream`."""
    import torch
    who = "particle_order"
    n = _drifter_arrays(who, px, py, status)
    it = field_bounds(grid, GO_T_POINTS)[0]
    need = C.c_longlong()
    check(_cabi.lib().dlesm_particle_order_scratch(n, C.byref(need)))
    with _on(stream):
        if perm is None:
            perm = torch.empty(n, dtype=torch.int32, device=px.device)
        nlive = torch.empty(1, dtype=torch.int32, device=px.device)
        scratch = torch.empty(max(need.value, 16), dtype=torch.uint8, device=px.device)
        if not (perm.is_cuda and perm.is_contiguous() and perm.dtype == torch.int32 and perm.numel() == n):
            raise _cabi.DlesmError(_cabi.EINVAL, "%s: perm is a contiguous int32 CUDA tensor of n elements" % who)
        check(_cabi.lib().dlesm_particle_order_f64(
            it.xstart, it.xstop, it.ystart, it.ystop, n, C.c_void_p(px.data_ptr()), C.c_void_p(py.data_ptr()),
            C.c_void_p(status.data_ptr()), C.c_void_p(perm.data_ptr()), C.c_void_p(nlive.data_ptr()),
            C.c_void_p(scratch.data_ptr()), need.value, _stream_ptr(stream)))
    return perm, nlive


def particle_permute(perm, arrays, out=None, stream=None):
    """out[a][k] = arrays[a][perm[k]] (dlesm_particle_permute) for any number of contiguous CUDA
    tensors of n elements of 4 or 8 bytes, eight to a launch; an index outside 0..n-1 leaves its slot as it was.  out: a
    list of tensors like `arrays`, or None for new ones.  Returns the list.  Asynchronous."""
    import torch
    who = "particle_permute"
    arrays = list(arrays)
    n = perm.numel()
    if not (perm.is_cuda and perm.is_contiguous() and perm.dtype == torch.int32):
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: perm is a contiguous int32 CUDA tensor" % who)
    if any(not (a.is_cuda and a.is_contiguous() and a.numel() == n and a.element_size() in (4, 8)) for a in arrays):
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: contiguous CUDA tensors of n elements of 4 or 8 bytes" % who)
    if out is None:
        with _on(stream):
            out = [torch.empty_like(a) for a in arrays]
    out = list(out)
    if len(out) != len(arrays) or any(not (o.is_cuda and o.is_contiguous() and o.numel() == n and o.dtype == a.dtype)
                                      for o, a in zip(out, arrays)):
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: out holds one tensor like each of arrays" % who)
    for first in range(0, len(arrays), 8):
        src, dst = arrays[first:first + 8], out[first:first + 8]
        k = len(src)
        check(_cabi.lib().dlesm_particle_permute(
            n, C.c_void_p(perm.data_ptr()), k, (C.c_void_p * k)(*[a.data_ptr() for a in src]),
            (C.c_void_p * k)(*[o.data_ptr() for o in dst]), (C.c_int * k)(*[a.element_size() for a in src]),
            _stream_ptr(stream)))
    return out


def particle_sort(px, py, status, un, carry=(), stream=None):
    """bring the particles into cell order in place: particle_order over the T internal region of
    un.grid, then px, py, status and every tensor of `carry` (contiguous CUDA tensors of one 4- or 8-byte element per
    particle: ages, identities, samples) gathered through the permutation and copied back.  Returns (perm, nlive); the live
    particles are the first nlive, so later steps may pass px[:k], py[:k], status[:k] for any k >= nlive.  Asynchronous."""
    arrays = [px, py, status] + list(carry)
    perm, nlive = particle_order(px, py, status, un.grid, stream=stream)
    with _on(stream):
        for a, b in zip(arrays, particle_permute(perm, arrays, stream=stream)):
            a.copy_(b)
    return perm, nlive


def cell_bin(px, py, status, grid, weights=(None,), out=None, perm=None, mode=_cabi.OUT_SET, alpha=1.0, stream=None):
    """the particles binned by cell (dlesm_cell_bin_f64): one output per entry of `weights`, the
    per-cell sum of that contiguous float64 CUDA tensor of one weight per particle -- None: 1.0, the cell's count, exact --
    over the DRIFTER_ACTIVE particles inside the T internal region of `grid`, the box particle_order uses, in the fixed
    order of section 6.19.  out: a list of contiguous float64 CUDA tensors of grid.ny x grid.nx, or None for new ones filled
    with zeros.  mode = OUT_SET stores alpha * sum in every cell of the region, OUT_ADD adds alpha * sum to the cells that
    hold a live particle.  perm: the particles' order by particle_order for the same grid (computed here when None).  Returns
    (out, unordered), unordered a one-element int32 CUDA tensor: 1 when perm was not in key order and the result is not
    defined.  Asynchronous, no synchronisation; the scratch is a tensor of the caching allocator made on `stream`."""
    import torch
    who = "cell_bin"
    n = _drifter_arrays(who, px, py, status)
    weights = list(weights)
    if not 1 <= len(weights) <= 8:
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: 1 to 8 weights" % who)
    if any(w is not None and not (w.is_cuda and w.is_contiguous() and w.dtype == torch.float64 and w.numel() == n)
           for w in weights):
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: a weight is None or a contiguous float64 CUDA tensor of n elements" % who)
    k = len(weights)
    it = field_bounds(grid, GO_T_POINTS)[0]
    need = C.c_longlong()
    check(_cabi.lib().dlesm_cell_bin_scratch(n, k, C.byref(need)))
    if perm is None:
        perm = particle_order(px, py, status, grid, stream=stream)[0]
    if not (perm.is_cuda and perm.is_contiguous() and perm.dtype == torch.int32 and perm.numel() == n):
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: perm is a contiguous int32 CUDA tensor of n elements" % who)
    with _on(stream):
        if out is None:
            out = [torch.zeros((grid.ny, grid.nx), dtype=torch.float64, device=px.device) for _ in weights]
        out = list(out)
        if len(out) != k or any(not (o.is_cuda and o.is_contiguous() and o.dtype == torch.float64 and
                                     o.numel() == grid.nx * grid.ny) for o in out):
            raise _cabi.DlesmError(_cabi.EINVAL, "%s: out holds one contiguous float64 CUDA tensor of ny x nx per weight" % who)
        unordered = torch.empty(1, dtype=torch.int32, device=px.device)
        scratch = torch.empty(max(need.value, 16), dtype=torch.uint8, device=px.device)
        check(_cabi.lib().dlesm_cell_bin_f64(
            int(mode), float(alpha), grid.nx, grid.ny, it.xstart, it.xstop, it.ystart, it.ystop, n, C.c_void_p(px.data_ptr()),
            C.c_void_p(py.data_ptr()), C.c_void_p(status.data_ptr()), C.c_void_p(perm.data_ptr()), k,
            (C.c_void_p * k)(*[w.data_ptr() if w is not None else None for w in weights]),
            (C.c_void_p * k)(*[o.data_ptr() for o in out]), C.c_void_p(unordered.data_ptr()), C.c_void_p(scratch.data_ptr()),
            need.value, _stream_ptr(stream)))
    return out, unordered


def _migrate_arrays(who, px, py, status, ids, payload):
    import torch
    n = _drifter_arrays(who, px, py, status)
    payload = list(payload)
    if not (ids.is_cuda and ids.is_contiguous() and ids.dtype == torch.int64 and ids.numel() == n):
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: ids is a contiguous int64 CUDA tensor of one element per slot" % who)
    if len(payload) > _cabi.MIGRATE_MAX_PAYLOAD or any(
            not (a.is_cuda and a.is_contiguous() and a.element_size() == 8 and a.numel() == n) for a in payload):
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: at most %d payload arrays, contiguous CUDA tensors of one 8-byte element "
                               "per slot" % (who, _cabi.MIGRATE_MAX_PAYLOAD))
    k = len(payload)
    return n, k, (C.c_void_p * max(k, 1))(*[a.data_ptr() for a in payload])


def _box_of(grid_or_field):
    grid = getattr(grid_or_field, "grid", grid_or_field)
    it = field_bounds(grid, GO_T_POINTS)[0]
    return grid, (it.xstart, it.xstop, it.ystart, it.ystop)


def migrate_message(cap, npayload=0, device="cuda"):
    """a message buffer of the particle migration for `cap` records with npayload payload words
    each: a uint8 CUDA tensor of dlesm_migrate_bytes bytes whose count is 0"""
    import torch
    need = C.c_longlong()
    check(_cabi.lib().dlesm_migrate_bytes(int(cap), int(npayload), C.byref(need)))
    m = torch.empty(need.value, dtype=torch.uint8, device=device)
    m[:16] = 0
    return m


def _migrate_scratch(n, device, scratch):
    import torch
    need = C.c_longlong()
    check(_cabi.lib().dlesm_migrate_scratch(n, C.byref(need)))
    if scratch is None:
        scratch = torch.empty(max(need.value, 16), dtype=torch.uint8, device=device)
    return scratch, scratch.numel()


def particle_pack(axis, px, py, status, ids, box, has_neighbour, shift_x, shift_y, cap, send, counts, payload=(), scratch=None,
                  stream=None):
    """the departures of one axis compacted into its two messages (dlesm_migrate_pack_f64).  axis:
    _cabi.MIGRATE_X (W, E) or MIGRATE_Y (S, N); box: (xstart, xstop, ystart, ystop); has_neighbour, shift_x, shift_y: two
    numbers each, low side first; send: two uint8 CUDA tensors of migrate_message's size; counts: an int32 CUDA tensor of 16
    elements, the dlesm_migrate_counts record.  status is the only particle array written.  Asynchronous."""
    who = "particle_pack"
    n, k, pp = _migrate_arrays(who, px, py, status, ids, payload)
    with _on(stream):
        scratch, nb = _migrate_scratch(n, px.device, scratch)
        check(_cabi.lib().dlesm_migrate_pack_f64(
            int(axis), *[int(b) for b in box], n, C.c_void_p(px.data_ptr()), C.c_void_p(py.data_ptr()),
            C.c_void_p(status.data_ptr()), C.c_void_p(ids.data_ptr()), pp, k, (C.c_int * 2)(*[int(bool(h)) for h in has_neighbour]),
            (C.c_int * 2)(*[int(v) for v in shift_x]), (C.c_int * 2)(*[int(v) for v in shift_y]), int(cap),
            (C.c_void_p * 2)(*[m.data_ptr() for m in send]), C.c_void_p(counts.data_ptr()), C.c_void_p(scratch.data_ptr()), nb,
            _stream_ptr(stream)))


def particle_unpack(axis, px, py, status, ids, box, cap, recv, counts, payload=(), scratch=None, stream=None):
    """the arrivals of one axis filled into the FREE slots (dlesm_migrate_unpack_f64): the records of
    recv[0] (from the low side), then those of recv[1], into the FREE slots in ascending order; arguments as particle_pack.
    Asynchronous."""
    who = "particle_unpack"
    n, k, pp = _migrate_arrays(who, px, py, status, ids, payload)
    with _on(stream):
        scratch, nb = _migrate_scratch(n, px.device, scratch)
        check(_cabi.lib().dlesm_migrate_unpack_f64(
            int(axis), *[int(b) for b in box], n, C.c_void_p(px.data_ptr()), C.c_void_p(py.data_ptr()),
            C.c_void_p(status.data_ptr()), C.c_void_p(ids.data_ptr()), pp, k, int(cap),
            (C.c_void_p * 2)(*[m.data_ptr() for m in recv]), C.c_void_p(counts.data_ptr()), C.c_void_p(scratch.data_ptr()), nb,
            _stream_ptr(stream)))


def particle_exchange(neighbour, send, recv, stream=None):
    """the transport of one axis (dlesm_migrate_exchange): send[d] to the 0-based rank neighbour[d],
    recv[d] from it; a negative neighbour gives an empty recv[d], the caller's own rank a device copy of send[d] into
    recv[1 - d].  Collective and synchronous, after waiting for the stream."""
    nb = send[0].numel()
    if any(m.numel() != nb or not m.is_cuda or not m.is_contiguous() for m in list(send) + list(recv)):
        raise _cabi.DlesmError(_cabi.EINVAL, "particle_exchange: four contiguous CUDA message buffers of one size")
    check(_cabi.lib().dlesm_migrate_exchange(
        (C.c_int * 2)(*[int(r) for r in neighbour]), (C.c_void_p * 2)(*[m.data_ptr() for m in send]),
        (C.c_void_p * 2)(*[m.data_ptr() for m in recv]), nb, _stream_ptr(stream)))


def migrate_neighbours(grid):
    """(neighbour, shift_x, shift_y) of this rank's tile for particle_migrate, each in the order W, E, S, N: the 0-based rank
    on that side from map_comms' send tables (-1: the edge of the global domain), and the integer a local coordinate gains
    on its way there: (my glob.xstart - my internal.xstart) - (the neighbour's), likewise in y."""
    # the edge strips' direction codes DLESM_IPLUS, _IMINUS, _JPLUS, _JMINUS: sent to the W, E, S and N neighbour
    side = {1: _cabi.MIGRATE_W, 2: _cabi.MIGRATE_E, 3: _cabi.MIGRATE_S, 4: _cabi.MIGRATE_N}
    neighbour, shift_x, shift_y = [-1] * 4, [0] * 4, [0] * 4
    tables = getattr(grid, "comm_tables", None)
    if grid.decomp is None or tables is None:
        return neighbour, shift_x, shift_y
    subs = grid.decomp.subdomains
    me = subs[parallel_mod.get_rank() - 1]
    for s in tables.sends():
        d = side.get(s["dir"])
        if d is None:
            continue
        o = subs[s["dest"]]
        neighbour[d] = s["dest"]
        shift_x[d] = (me.glob.xstart - me.internal.xstart) - (o.glob.xstart - o.internal.xstart)
        shift_y[d] = (me.glob.ystart - me.internal.ystart) - (o.glob.ystart - o.internal.ystart)
    return neighbour, shift_x, shift_y


class MigrateError(_cabi.DlesmError):
    """particle_migrate lost particles (dropped) or met a bad message; .counts holds the record"""


def particle_migrate(px, py, status, ids, grid_or_field, payload=(), cap=None, work=None, stream=None):
    """hand the particles that have left this rank's tile to the neighbouring ranks and take theirs (dlesm_migrate_f64,
    DESIGN.md section 6.21): phase X (W, E), then phase Y (S, N), so a corner crossing arrives within the call.  px, py,
    status as drifter_step, of the set's capacity n, slots without a particle DRIFTER_FREE; ids: a contiguous int64 CUDA tensor,
    the identity that travels with a particle (dispersal_step takes its low 32 bits); payload: up to 4 contiguous CUDA tensors
    of one 8-byte element per slot that travel too.  The box is the T internal region of the grid, the neighbours and shifts
    are migrate_neighbours(grid).  cap: the records one message holds (the same on every rank; default min(n, 65536), at
    least 1); departures beyond it stay LEFT and go with a later call.  work: a uint8 CUDA tensor of dlesm_migrate_work bytes
    to reuse, or None.  Returns the _cabi.MigrateCounts record after the call; raises MigrateError if particles were dropped
    for want of FREE slots or a message was bad.  A particle that crosses loses the rest of the substeps of the step that
    made it LEFT: step with nsub = 1 between migrations for no lag.  Collective and synchronous."""
    import torch
    who = "particle_migrate"
    n, k, pp = _migrate_arrays(who, px, py, status, ids, payload)
    grid, box = _box_of(grid_or_field)
    cap = max(1, min(n, 65536)) if cap is None else int(cap)
    neighbour, shift_x, shift_y = migrate_neighbours(grid)
    need = C.c_longlong()
    check(_cabi.lib().dlesm_migrate_work(n, cap, k, C.byref(need)))
    with _on(stream):
        if work is None:
            work = torch.empty(need.value, dtype=torch.uint8, device=px.device)
        counts = torch.empty(16, dtype=torch.int32, device=px.device)
        check(_cabi.lib().dlesm_migrate_f64(
            *box, n, C.c_void_p(px.data_ptr()), C.c_void_p(py.data_ptr()), C.c_void_p(status.data_ptr()),
            C.c_void_p(ids.data_ptr()), pp, k, (C.c_int * 4)(*neighbour), (C.c_int * 4)(*shift_x), (C.c_int * 4)(*shift_y), cap,
            C.c_void_p(counts.data_ptr()), C.c_void_p(work.data_ptr()), work.numel(), _stream_ptr(stream)))
        host = counts.cpu().numpy()
    rec = _cabi.MigrateCounts.from_buffer_copy(host.tobytes())
    if rec.dropped or rec.bad_message:
        e = MigrateError(_cabi.EINVAL, "%s: %d arrivals dropped for want of FREE slots, bad_message = %d" %
                         (who, rec.dropped, rec.bad_message))
        e.counts = rec
        raise e
    return rec


class ReleaseError(_cabi.DlesmError):
    """particle_release dropped particles for want of FREE slots, clamped a source or met a bad one; .counts holds the record"""


def release_sources(x, y, rx, ry, first_id, count=0, tag=None, device="cuda"):
    """the device table of particle sources: an int64 CUDA tensor of nsources x 8 words, one
    dlesm_release_source a row -- x, y, rx, ry as the bits of doubles, next_id, count, tag, pad.  x, y: the centres in GLOBAL
    index coordinates; rx, ry: the half-widths in cells (0: a point source); first_id: the id of each source's first
    particle -- give every source a range of its own; count: the particles wanted at the next call; tag: 8 bytes stored with
    every particle of the source (default: the source's number).  Every argument is a number or a sequence of nsources; every
    rank builds the same table.  Column 5 of the tensor may be rewritten between calls to change the rate."""
    import numpy as np
    import torch
    cols = [np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (x, y, rx, ry)]
    ns = max([c.size for c in cols] + [np.atleast_1d(np.asarray(v)).size for v in (first_id, count)])
    if ns > _cabi.RELEASE_MAX_SOURCES:
        raise _cabi.DlesmError(_cabi.EINVAL, "release_sources: %d sources (at most %d)" % (ns, _cabi.RELEASE_MAX_SOURCES))
    table = np.zeros((ns, 8), dtype=np.int64)
    for k, c in enumerate(cols):
        table[:, k] = np.broadcast_to(c, (ns,)).copy().view(np.int64)
    table[:, 4] = np.broadcast_to(np.asarray(first_id, dtype=np.int64), (ns,))
    table[:, 5] = np.broadcast_to(np.asarray(count, dtype=np.int64), (ns,))
    table[:, 6] = np.arange(ns) if tag is None else np.broadcast_to(np.asarray(tag, dtype=np.int64), (ns,))
    return torch.from_numpy(table).to(device)


def particle_release(sources, px, py, status, ids, grid_or_field, seed, tick=0, tick_dev=None, tag=None, born=None,
                     max_count=None, scratch=None, stream=None, wait=True):
    """create this call's particles of every source in the FREE slots of the set (dlesm_release_f64).
    sources: release_sources' table, the same on every rank; its next_id column advances by what each source gave.  px, py,
    status, ids as particle_migrate.  The box is the T internal region of the grid, offx = glob.xstart - internal.xstart of this
    rank's subdomain (0 without a decomposition), the difference migrate_neighbours uses; a candidate outside this rank's tile
    is another rank's.  seed, tick, tick_dev as dispersal_step; tag, born: None or contiguous int64 CUDA tensors of one element
    per slot that receive the source's tag and tick + *tick_dev.  max_count: the most one source may give in a call (default:
    the largest count of the table, read once from the device -- pass it for a captured loop).  scratch: a uint8 CUDA tensor
    of dlesm_release_scratch bytes to reuse, or None.  wait=True returns the _cabi.ReleaseCounts record after the call and raises
    ReleaseError if particles were dropped, a source was clamped or a source was bad; wait=False returns the record on the
    device, an int32 CUDA tensor of 16 elements, without a synchronisation."""
    import torch
    who = "particle_release"
    n = _drifter_arrays(who, px, py, status)

    def slots(t):
        return t.is_cuda and t.is_contiguous() and t.dtype == torch.int64 and t.numel() == n

    def ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    if not slots(ids) or any(t is not None and not slots(t) for t in (tag, born)):
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: ids, tag and born are contiguous int64 CUDA tensors of one element per slot" % who)
    if not (sources.is_cuda and sources.is_contiguous() and sources.dtype == torch.int64 and sources.dim() == 2 and
            sources.shape[1] == 8):
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: sources is release_sources' int64 CUDA tensor of nsources x 8" % who)
    if tick_dev is not None and not (tick_dev.is_cuda and tick_dev.dtype == torch.int64 and tick_dev.numel() == 1):
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: tick_dev is a one-element int64 CUDA tensor" % who)
    ns = sources.shape[0]
    grid, box = _box_of(grid_or_field)
    offx = offy = 0
    if grid.decomp is not None:
        me = grid.decomp.subdomains[parallel_mod.get_rank() - 1]
        offx, offy = me.glob.xstart - me.internal.xstart, me.glob.ystart - me.internal.ystart
    if max_count is None:
        max_count = max(1, int(sources[:, 5].max().item())) if ns else 1
    seed = int(seed) & 0xffffffffffffffff
    need = C.c_longlong()
    check(_cabi.lib().dlesm_release_scratch(n, ns, int(max_count), C.byref(need)))
    with _on(stream):
        if scratch is None:
            scratch = torch.empty(max(need.value, 16), dtype=torch.uint8, device=px.device)
        counts = torch.empty(16, dtype=torch.int32, device=px.device)
        check(_cabi.lib().dlesm_release_f64(
            grid.nx, grid.ny, *box, offx, offy, grid.tmask_device_ptr, ptr(sources), ns, int(max_count),
            seed - (1 << 64) if seed >> 63 else seed, int(tick), ptr(tick_dev), n, ptr(px), ptr(py), ptr(status), ptr(ids),
            ptr(tag), ptr(born), ptr(counts), ptr(scratch), scratch.numel(), _stream_ptr(stream)))
        if not wait:
            return counts
        host = counts.cpu().numpy()
    rec = _cabi.ReleaseCounts.from_buffer_copy(host.tobytes())
    if rec.dropped or rec.clamped or rec.bad_source:
        e = ReleaseError(_cabi.EINVAL, "%s: %d particles dropped for want of FREE slots, %d sources clamped to max_count, %d "
                         "bad sources" % (who, rec.dropped, rec.clamped, rec.bad_source))
        e.counts = rec
        raise e
    return rec


TRACER_SCHEMES = {"upwind": _cabi.TRACER_UPWIND, "muscl": _cabi.TRACER_MUSCL, "hancock": _cabi.TRACER_HANCOCK}


def invoke_nemolite_coupled_step_dm(params, scheme, c_out, c_in, ssha, ssha_u, ssha_v, ua, va, un, vn, ht, hu, hv, sshn_t, sshn_u,
                                    sshn_v, ssh_bc=None, stream=None, skip_land=False):
    """one coupled time step on a decomposed grid (dlesm_nemolite_coupled_step_dm): the flow step of
    invoke_nemolite_step_dm and the tracer sweep of `scheme` ("upwind" | "muscl" | "hancock") with rdt = params.rdt, c_in
    carried to c_out by the level-n transports into the new water column, then ONE exchange of ssha, ssha_u, ssha_v, ua, va
    and every c_out.  c_out and c_in are lists of T-point fields (both empty: the flow step alone).  The flow inputs need valid
    depth-1 halos, corners included; c_in depth-1 halos for "upwind", c_in and the grid's mask depth-2 halos for the limited
    schemes (grid_mod.exchange_mask_halos fills the mask's); every output leaves with halos of the grid's halo_width.
    Collective.  Stops on a halo_width other than 1 or 2, on a limited scheme with halo_width 1, and when the grid's Coriolis
    parameter was never set.  ssh_bc and skip_land as invoke_nemolite_step_dm."""
    who = "invoke_nemolite_coupled_step_dm"
    g = ssha.grid
    if scheme not in TRACER_SCHEMES:
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: scheme %r (one of %s)" % (who, scheme, ", ".join(TRACER_SCHEMES)))
    pin, pout, n = _tracer_ptrs(who, c_out, c_in)
    hw = getattr(g, "halo_width", 1)
    if hw not in (1, 2):
        raise _cabi.GoceanStop(_cabi.EABORT, "%s: the grid has halo_width %d; the step exchanges depth-1 or depth-2 halos: "
                                             "decompose the grid with halo_width = 1 or 2" % (who, hw))
    if hw == 1 and scheme != "upwind" and n:
        raise _cabi.GoceanStop(_cabi.EABORT, "%s: the grid has halo_width 1; the %s scheme reads two cells and exchanges "
                                             "depth-2 halos: decompose the grid with halo_width = 2" % (who, scheme))
    mg = _momentum_grid(g, who)
    if getattr(g, "comm_tables", None) is None:
        raise _cabi.DlesmError(_cabi.EINVAL, "%s: the grid has no message tables (grid_init after decompose)" % who)
    obc = None if ssh_bc is None else open_boundary(g).handle
    check(_cabi.lib().dlesm_nemolite_coupled_step_dm(
        grid_mod.halo_plan(g), wet_plan(g).handle if skip_land else None, TRACER_SCHEMES[scheme], C.byref(params), C.byref(mg),
        C.c_void_p(g.area_t_device.data_ptr()), g.nx, g.ny, C.byref(ssha.internal), C.byref(ua.internal), C.byref(va.internal),
        obc, 0.0 if ssh_bc is None else float(ssh_bc),
        *[f.device_ptr for f in (un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v, ssha, ssha_u, ssha_v, ua, va)], pin, pout, n,
        _stream_ptr(stream)))


def invoke_jacobi5_masked(out_fld, in_fld, stream=None):
    """the masked Jacobi kernel (metadata: GO_GRID_MASK_T): the PSy layer hands the kernel the
    grid's T mask, here its device mirror"""
    g, it = out_fld.grid, out_fld.internal
    check(_cabi.lib().dlesm_stencil5_masked_f64(in_fld.device_ptr, out_fld.device_ptr, g.tmask_device_ptr, g.nx,
                                                g.ny, it.xstart, it.xstop, it.ystart, it.ystop,
                                                _stream_ptr(stream)))


def autotune_jacobi5(out_fld, in_fld, stream=None):
    """optional planning call: measure the launch shapes of invoke_jacobi5 for this field geometry
    once (each trial is the same valid step in -> out) and keep the fastest"""
    g, it = out_fld.grid, out_fld.internal
    check(_cabi.lib().dlesm_stencil5_autotune_f64(in_fld.device_ptr, out_fld.device_ptr, g.nx, g.ny,
                                                  it.xstart, it.xstop, it.ystart, it.ystop,
                                                  _stream_ptr(stream)))


def planned_shape_jacobi5(out_fld):
    """(waves per workgroup, tiles per row, rows per tile, non-temporal stores) for this geometry; the first
    three are 0 before autotune_jacobi5 has run for it"""
    g, it = out_fld.grid, out_fld.internal
    a, b, c, d = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    check(_cabi.lib().dlesm_stencil5_planned_shape(g.nx, it.xstart, it.xstop, it.ystart, it.ystop, C.byref(a), C.byref(b),
                                                   C.byref(c), C.byref(d)))
    return a.value, b.value, c.value, d.value


def invoke_jacobi5_x2(out_fld, in_fld, ebox=None, stream=None):
    """TWO Jacobi steps in one sweep: out = J(t) on out_fld%internal, t = J(in) on `ebox`
    (default: the same box, i.e. a fixed boundary ring) and in elsewhere"""
    g, it = out_fld.grid, out_fld.internal
    e = ebox if ebox is not None else it.box()
    check(_cabi.lib().dlesm_stencil5_x2_f64(in_fld.device_ptr, out_fld.device_ptr, g.nx, g.ny,
                                            it.xstart, it.xstop, it.ystart, it.ystop, *e,
                                            _stream_ptr(stream)))


def invoke_jacobi5_multi(out_fld, in_fld, nsteps, ebox=None, grow=(0, 0, 0, 0), stream=None):
    """nsteps (2..8) Jacobi steps in one sweep over out_fld%internal; `ebox` is the last stage
    box (default: the same box, a fixed boundary ring), `grow` the (W, E, S, N) flags"""
    g, it = out_fld.grid, out_fld.internal
    e = ebox if ebox is not None else it.box()
    check(_cabi.lib().dlesm_stencil5_multi_f64(in_fld.device_ptr, out_fld.device_ptr, g.nx, g.ny, nsteps,
                                               it.xstart, it.xstop, it.ystart, it.ystop, *e, *grow,
                                               _stream_ptr(stream)))


def invoke_jacobi5_multi_dm(out_fld, in_fld, nsteps, stream=None):
    """nsteps distributed Jacobi steps with ONE depth-nsteps exchange (hidden behind the interior);
    the grid must have been decomposed with halo_width = nsteps"""
    g, it = out_fld.grid, out_fld.internal
    check(_cabi.lib().dlesm_jacobi5_multi_step_dm(grid_mod.halo_plan(g), in_fld.device_ptr,
                                                  out_fld.device_ptr, g.nx, g.ny, nsteps, it.xstart,
                                                  it.xstop, it.ystart, it.ystop, _stream_ptr(stream)))


def invoke_jacobi5_dm(out_fld, in_fld, stream=None):
    """distributed step: frame, then exchange(out) hidden behind the interior"""
    g, it = out_fld.grid, out_fld.internal
    plan = grid_mod.halo_plan(g)
    check(_cabi.lib().dlesm_jacobi5_step_dm(plan, in_fld.device_ptr, out_fld.device_ptr, g.nx, g.ny,
                                            it.xstart, it.xstop, it.ystart, it.ystop,
                                            _stream_ptr(stream)))


def invoke_jacobi5_dm_pipelined(out_fld, in_fld, stream=None):
    """the distributed step inside a time loop: returns with the exchange of `out` in flight; the
    next such step waits for it on the device.  Call halo_join(grid) before anything else reads halos."""
    g, it = out_fld.grid, out_fld.internal
    check(_cabi.lib().dlesm_jacobi5_step_dm_pipelined(grid_mod.halo_plan(g), in_fld.device_ptr, out_fld.device_ptr,
                                                      g.nx, g.ny, it.xstart, it.xstop, it.ystart, it.ystop,
                                                      _stream_ptr(stream)))


def invoke_jacobi5_residual(out_fld, in_fld, norm="max", stream=None):
    """the Jacobi step of invoke_jacobi5 (same `out`, bit for bit) that also says how far it moved the field over
    out_fld%internal on all ranks: max|out - in| (norm="max") or sqrt(SUM (out - in)**2) (norm="l2").  Synchronous: what a
    solver checks every few steps to know when to stop.  On a decomposed grid it first joins a pipelined step's exchange
    (`in`'s halos) and leaves `out` with its depth-1 halos exchanged, as invoke_jacobi5_dm does."""
    codes = {"max": _cabi.NORM_MAX, "l2": _cabi.NORM_SUMSQ}
    if norm not in codes:
        raise ValueError(f"invoke_jacobi5_residual: norm {norm!r} is not 'max' or 'l2'")
    g, it = out_fld.grid, out_fld.internal
    dm = parallel_mod.get_num_ranks() > 1
    if dm:
        halo_join(g, stream)

    def step(res, s):                                       # the sweep, then the exchange, then _fetch_record's copy
        check(_cabi.lib().dlesm_stencil5_resid_f64(in_fld.device_ptr, out_fld.device_ptr, g.nx, g.ny, it.xstart, it.xstop,
                                                   it.ystart, it.ystop, codes[norm], res, s))
        if dm:
            out_fld.halo_exchange(1, stream=stream)         # (None: the current stream, which is `stream` in there)
    val = C.c_double.from_buffer_copy(_fetch_record(stream, out_fld.data.device, 1, step)).value
    return parallel_mod.global_max(val) if norm == "max" else math.sqrt(parallel_mod.global_sum(val))


def run_health(fields, names, masks=None, max_abs=None, stream=None):
    """the check a time loop makes every few steps (NEMO's stp_ctl): ONE field_stats call over the fields' internal regions
    (masks as in field_mod.field_stats); returns the list of FieldStats, the same on every rank.  Raises DlesmError -- on
    every rank -- when a field holds a NaN or an infinity on any rank, or when max(|min|, |max|) of field k exceeds
    max_abs[k] (max_abs: None, one bound for all fields, or one entry per field, None = no bound).  The message names the
    field, the lowest rank (1-based, parallel_mod.get_rank) that holds an offending cell and the local 1-based (i, j) of
    its first such cell."""
    from . import field_mod
    fields, names = list(fields), list(names)
    if len(names) != len(fields):
        raise ValueError(f"run_health: {len(names)} names for {len(fields)} fields")
    if max_abs is None or not isinstance(max_abs, (list, tuple)):
        max_abs = [max_abs] * len(fields)
    if len(max_abs) != len(fields):
        raise ValueError(f"run_health: {len(max_abs)} bounds for {len(fields)} fields")
    stats = field_mod.field_stats(fields, masks, stream)
    mlist = field_mod._mask_list(masks, len(fields))
    for k, (st, name) in enumerate(zip(stats, names)):
        if st.nonfinite > 0:
            what, value, why = "nonfinite", None, f"{st.nonfinite} cell(s) NaN or infinite"
        elif max_abs[k] is not None and max(abs(st.min), abs(st.max)) > max_abs[k] and st.count > st.nonfinite:
            value = st.max if abs(st.max) >= abs(st.min) else st.min
            what, why = "equal", f"|{value!r}| exceeds {max_abs[k]!r}"
        else:
            continue
        here = field_mod.field_locate(fields[k], what, value, mlist[k], stream)
        i, j = here or (0, 0)
        rank, i, j = parallel_mod._owner(here is not None, i, j) or (parallel_mod.get_rank(), 0, 0)
        raise _cabi.DlesmError(_cabi.EABORT, f"run_health: field {name}: {why}; first at local (i, j) = ({i}, {j}) on rank {rank}")
    return stats


def halo_connect_peers(grid, nfields=1):
    """collective: connect the grid's plan to the neighbours' mailboxes (grid_mod.connect_peers) -- the distributed
    Jacobi steps then exchange with stores over xGMI instead of an RCCL group"""
    grid_mod.connect_peers(grid, nfields)


def halo_join(grid, stream=None):
    """order `stream` behind the exchange a pipelined step left in flight"""
    check(_cabi.lib().dlesm_halo_plan_join(grid_mod.halo_plan(grid), _stream_ptr(stream)))


def shallow_params(dx, dy, dt):
    """constants of the shallow-water step: tdt = 2*dt (leapfrog)"""
    tdt = dt + dt
    return SwParams(fsdx=4.0 / dx, fsdy=4.0 / dy, tdts8=tdt / 8.0, tdtsdx=tdt / dx, tdtsdy=tdt / dy)


def _shallow_head(params, alpha, plan, fields):
    """what every shallow-water entry takes first: [plan,] params, [alpha,] and the extents of the arrays (p is fields[2])"""
    g = fields[2].grid
    return (() if plan is None else (plan,)) + (C.byref(params),) + (() if alpha is None else (float(alpha),)) + (g.nx, g.ny)


def _shallow_box(entry, params, alpha, plan, fields, stream):
    """the body of the shallow-water wrappers whose C entry takes the box as four integers: the internal region of p, then the
    9 or 12 arrays and the stream"""
    it = fields[2].internal
    check(getattr(_cabi.lib(), entry)(*_shallow_head(params, alpha, plan, fields), it.xstart, it.xstop, it.ystart, it.ystop,
                                      *[f.device_ptr for f in fields], _stream_ptr(stream)))


def _shallow_region(entry, params, alpha, fields, stream):
    """the same for the periodic entries, which take p's internal region and the grid's boundary conditions in x and y"""
    p = fields[2]
    check(getattr(_cabi.lib(), entry)(*_shallow_head(params, alpha, None, fields), C.byref(p.internal),
                                      *p.grid.boundary_conditions[:2], *[f.device_ptr for f in fields], _stream_ptr(stream)))


def invoke_shallow_step(params, u, v, p, uold, vold, pold, unew, vnew, pnew, stream=None):
    _shallow_box("dlesm_shallow_step_f64", params, None, None, (u, v, p, uold, vold, pold, unew, vnew, pnew), stream)


def invoke_shallow_step_x2(params, u, v, p, uold, vold, pold, unew, vnew, pnew, unew2, vnew2, pnew2, stream=None):
    """TWO leapfrog steps in one launch (dlesm_shallow_step_x2_f64): level n+1 into unew / vnew / pnew, level n+2 into
    unew2 / vnew2 / pnew2 -- the bits of two invoke_shallow_step calls at 48 instead of 72 B/cell/step.  Time loop:
    (cur, old, new1, new2) <- (new2, new1, old, cur) after every call."""
    _shallow_box("dlesm_shallow_step_x2_f64", params, None, None, (u, v, p, uold, vold, pold, unew, vnew, pnew, unew2, vnew2, pnew2), stream)


def invoke_shallow_step_smooth_x2(params, alpha, u, v, p, uold, vold, pold, unew2, vnew2, pnew2, uold2, vold2, pold2, stream=None):
    """TWO filtered leapfrog steps (update + time_smooth, twice) in one launch (dlesm_shallow_step_smooth_x2_f64): level n+2 into
    unew2.., the filtered level n+1 into uold2..; inputs untouched.  Time loop: ping-pong (cur, old) <-> (unew2.., uold2..)."""
    _shallow_box("dlesm_shallow_step_smooth_x2_f64", params, alpha, None, (u, v, p, uold, vold, pold, unew2, vnew2, pnew2, uold2, vold2, pold2), stream)


def invoke_shallow_step_sw(params, u, v, p, uold, vold, pold, unew, vnew, pnew, stream=None):
    """the SW-offset form (the GOcean `shallow` staggering); periodic models follow it with
    apply_periodic_halos on the three new fields"""
    _shallow_box("dlesm_shallow_step_sw_f64", params, None, None, (u, v, p, uold, vold, pold, unew, vnew, pnew), stream)


# ---- the GOcean `shallow` kernels one by one: what an unmodified generated PSy layer calls ----------------
def _kernel_box(out_fld, box):
    """the loop bounds of the nest: the written field's internal region (ITERATES_OVER = GO_INTERNAL_PTS,
    kernel_mod.f90:28-50) unless the caller's PSy layer runs the kernel over another box"""
    return tuple(box) if box is not None else out_fld.internal.box()


def invoke_compute_cu(cu, p, u, box=None, stream=None):
    """`call compute_cu_code(ji, jj, cu%data, p%data, u%data)` over cu%internal"""
    g = cu.grid
    check(_cabi.lib().dlesm_compute_cu_f64(g.offset, g.nx, g.ny, *_kernel_box(cu, box), cu.device_ptr, p.device_ptr,
                                           u.device_ptr, _stream_ptr(stream)))


def invoke_compute_cv(cv, p, v, box=None, stream=None):
    g = cv.grid
    check(_cabi.lib().dlesm_compute_cv_f64(g.offset, g.nx, g.ny, *_kernel_box(cv, box), cv.device_ptr, p.device_ptr,
                                           v.device_ptr, _stream_ptr(stream)))


def invoke_compute_z(z, p, u, v, box=None, stream=None):
    """fsdx = 4/dx, fsdy = 4/dy from the grid (the kernel's GO_GRID_DX_CONST / GO_GRID_DY_CONST arguments)"""
    g = z.grid
    check(_cabi.lib().dlesm_compute_z_f64(g.offset, g.nx, g.ny, *_kernel_box(z, box), 4.0 / g.dx, 4.0 / g.dy,
                                          z.device_ptr, p.device_ptr, u.device_ptr, v.device_ptr, _stream_ptr(stream)))


def invoke_compute_h(h, p, u, v, box=None, stream=None):
    g = h.grid
    check(_cabi.lib().dlesm_compute_h_f64(g.offset, g.nx, g.ny, *_kernel_box(h, box), h.device_ptr, p.device_ptr,
                                          u.device_ptr, v.device_ptr, _stream_ptr(stream)))


def invoke_compute_unew(unew, uold, z, cv, h, tdt, box=None, stream=None):
    """tdt = 2*dt in a leapfrog step; tdts8 = tdt/8, tdtsdx = tdt/dx"""
    g = unew.grid
    check(_cabi.lib().dlesm_compute_unew_f64(g.offset, g.nx, g.ny, *_kernel_box(unew, box), tdt / 8.0, tdt / g.dx,
                                             unew.device_ptr, uold.device_ptr, z.device_ptr, cv.device_ptr,
                                             h.device_ptr, _stream_ptr(stream)))


def invoke_compute_vnew(vnew, vold, z, cu, h, tdt, box=None, stream=None):
    g = vnew.grid
    check(_cabi.lib().dlesm_compute_vnew_f64(g.offset, g.nx, g.ny, *_kernel_box(vnew, box), tdt / 8.0, tdt / g.dy,
                                             vnew.device_ptr, vold.device_ptr, z.device_ptr, cu.device_ptr,
                                             h.device_ptr, _stream_ptr(stream)))


def invoke_compute_pnew(pnew, pold, cu, cv, tdt, box=None, stream=None):
    g = pnew.grid
    check(_cabi.lib().dlesm_compute_pnew_f64(g.offset, g.nx, g.ny, *_kernel_box(pnew, box), tdt / g.dx, tdt / g.dy,
                                             pnew.device_ptr, pold.device_ptr, cu.device_ptr, cv.device_ptr,
                                             _stream_ptr(stream)))


def invoke_time_smooth(field, field_new, field_old, alpha, box=None, stream=None):
    """field_old = field + alpha*(field_new - 2*field + field_old) over field_old%internal"""
    g = field_old.grid
    check(_cabi.lib().dlesm_time_smooth_f64(g.nx, g.ny, *_kernel_box(field_old, box), float(alpha), field.device_ptr,
                                            field_new.device_ptr, field_old.device_ptr, _stream_ptr(stream)))


def invoke_shallow_kernel_sequence(tdt, u, v, p, uold, vold, pold, cu, cv, z, h, unew, vnew, pnew, stream=None):
    """One time step the way a generated PSy layer runs it: seven loop nests, every intermediate through HBM
    (224 B/cell).  Non-periodic grids: cu, cv, z, h over the internal region grown towards their consumers (all
    operands stay inside the boundary ring); periodic (SW-offset) grids: over the internal region, followed by
    their periodic copies, as the benchmark does.  Bit-identical to invoke_shallow_step / invoke_shallow_step_sw."""
    g = p.grid
    xs, xe, ys, ye = p.internal.box()
    periodic = GO_BC_PERIODIC_ in g.boundary_conditions[:2]
    if periodic:
        grown = dict(cu=None, cv=None, z=None, h=None)
    elif g.offset == grid_mod.GO_OFFSET_NE:
        grown = dict(cu=(xs - 1, xe, ys, ye + 1), cv=(xs, xe + 1, ys - 1, ye), z=(xs - 1, xe, ys - 1, ye),
                     h=(xs, xe + 1, ys, ye + 1))
    else:
        grown = dict(cu=(xs, xe + 1, ys - 1, ye), cv=(xs - 1, xe, ys, ye + 1), z=(xs, xe + 1, ys, ye + 1),
                     h=(xs - 1, xe, ys - 1, ye))
    invoke_compute_cu(cu, p, u, grown["cu"], stream)
    invoke_compute_cv(cv, p, v, grown["cv"], stream)
    invoke_compute_z(z, p, u, v, grown["z"], stream)
    invoke_compute_h(h, p, u, v, grown["h"], stream)
    if periodic:
        apply_periodic_halos_multi([cu, cv, z, h], stream)
    invoke_compute_unew(unew, uold, z, cv, h, tdt, None, stream)
    invoke_compute_vnew(vnew, vold, z, cu, h, tdt, None, stream)
    invoke_compute_pnew(pnew, pold, cu, cv, tdt, None, stream)


GO_BC_PERIODIC_ = grid_mod.GO_BC_PERIODIC


def invoke_shallow_step_sw_periodic(params, u, v, p, uold, vold, pold, unew, vnew, pnew, stream=None):
    """the SW-offset step over the internal region AND the periodic copies of the three new fields in one launch
    (== invoke_shallow_step_sw + apply_periodic_halos_multi, bit for bit)"""
    _shallow_region("dlesm_shallow_step_sw_periodic_f64", params, None, (u, v, p, uold, vold, pold, unew, vnew, pnew), stream)


def invoke_shallow_step_sw_x2_periodic(params, u, v, p, uold, vold, pold, unew, vnew, pnew, unew2, vnew2, pnew2, stream=None):
    """two steps of the SW-offset periodic model in one launch (== two invoke_shallow_step_sw_periodic calls)"""
    _shallow_region("dlesm_shallow_step_sw_x2_periodic_f64", params, None, (u, v, p, uold, vold, pold, unew, vnew, pnew, unew2, vnew2, pnew2), stream)


def invoke_shallow_step_sw_smooth_x2_periodic(params, alpha, u, v, p, uold, vold, pold, unew2, vnew2, pnew2, uold2, vold2, pold2, stream=None):
    """two WHOLE time steps of the GOcean `shallow` benchmark (update + time_smooth + periodic images, twice) in one launch:
    level n+2 into unew2.., the filtered level n+1 into uold2..; ping-pong between the two sextets"""
    _shallow_region("dlesm_shallow_step_sw_smooth_x2_periodic_f64", params, alpha, (u, v, p, uold, vold, pold, unew2, vnew2, pnew2, uold2, vold2, pold2), stream)


def invoke_shallow_step_smooth(params, alpha, u, v, p, uold, vold, pold, unew, vnew, pnew, stream=None):
    """one whole leapfrog step of the GOcean benchmark in one launch (NE offset): the u/v/h update + time_smooth of the
    old level in place (== invoke_shallow_step + 3 x invoke_time_smooth, bit for bit).  Afterwards rotate u <- unew."""
    _shallow_box("dlesm_shallow_step_smooth_f64", params, alpha, None, (u, v, p, uold, vold, pold, unew, vnew, pnew), stream)


def invoke_shallow_step_sw_smooth_periodic(params, alpha, u, v, p, uold, vold, pold, unew, vnew, pnew, stream=None):
    """the same for the SW-offset periodic model: step + time_smooth + the periodic images of the new and of the filtered
    old level, one launch"""
    _shallow_region("dlesm_shallow_step_sw_smooth_periodic_f64", params, alpha, (u, v, p, uold, vold, pold, unew, vnew, pnew), stream)


def apply_periodic_halos(fld, stream=None):
    """the periodic-boundary copies of a field (field_mod.f90:1394-1464), on the device"""
    g = fld.grid
    check(_cabi.lib().dlesm_periodic_halos_apply_f64(fld.device_ptr, g.nx, g.ny, C.byref(fld.internal),
                                                     g.boundary_conditions[0], g.boundary_conditions[1],
                                                     _stream_ptr(stream)))


def apply_periodic_halos_multi(fields, stream=None):
    """the periodic copies of several fields of one grid and internal region in two launches"""
    g = fields[0].grid
    arr = (C.c_void_p * len(fields))(*[f.device_ptr.value for f in fields])
    check(_cabi.lib().dlesm_periodic_halos_apply_multi_f64(arr, len(fields), g.nx, g.ny, C.byref(fields[0].internal),
                                                           g.boundary_conditions[0], g.boundary_conditions[1],
                                                           _stream_ptr(stream)))


def autotune_shallow(params, u, v, p, uold, vold, pold, unew, vnew, pnew, stream=None):
    """optional planning call for invoke_shallow_step: time the launch shapes / cache policies once
    for this field geometry (each trial is the same valid step) and keep the fastest"""
    _shallow_box("dlesm_shallow_autotune_f64", params, None, None, (u, v, p, uold, vold, pold, unew, vnew, pnew), stream)


def autotune_shallow_sw(params, u, v, p, uold, vold, pold, unew, vnew, pnew, stream=None):
    """the planning call of the SW-offset step (invoke_shallow_step_sw / invoke_shallow_step_sw_periodic)"""
    _shallow_box("dlesm_shallow_autotune_sw_f64", params, None, None, (u, v, p, uold, vold, pold, unew, vnew, pnew), stream)


def invoke_shallow_step_dm(params, u, v, p, uold, vold, pold, unew, vnew, pnew, stream=None):
    """distributed form: frame of the new fields, one grouped exchange of all three behind the
    interior; unew, vnew, pnew leave with valid halos"""
    _shallow_box("dlesm_shallow_step_dm", params, None, grid_mod.halo_plan(p.grid), (u, v, p, uold, vold, pold, unew, vnew, pnew), stream)


def invoke_shallow_step_dm_pipelined(params, u, v, p, uold, vold, pold, unew, vnew, pnew, stream=None):
    """the distributed shallow-water step inside a time loop: returns with the exchange of the new
    fields in flight; the next such step waits for it on the device.  halo_join(grid) before anything
    else reads their halos."""
    _shallow_box("dlesm_shallow_step_dm_pipelined", params, None, grid_mod.halo_plan(p.grid), (u, v, p, uold, vold, pold, unew, vnew, pnew), stream)


def invoke_shallow_step_smooth_dm(params, alpha, u, v, p, uold, vold, pold, unew, vnew, pnew, stream=None, pipelined=False):
    """the distributed step with the Asselin filter of the old level folded in (joined or time-loop form)"""
    _shallow_box("dlesm_shallow_step_smooth_dm_pipelined" if pipelined else "dlesm_shallow_step_smooth_dm", params, alpha,
                 grid_mod.halo_plan(p.grid), (u, v, p, uold, vold, pold, unew, vnew, pnew), stream)


def _x2_dm_plan(g, who):
    """the plan of a grid decomposed with halo_width = 2 (the two-step distributed entries need depth-2 halos)"""
    if getattr(g, "halo_width", 1) != 2:
        raise _cabi.DlesmError(_cabi.EINVAL, f"{who}: the grid has halo_width {getattr(g, 'halo_width', 1)}; two steps per "
                                             "call need a grid decomposed with halo_width = 2")
    if getattr(g, "comm_tables", None) is None:
        raise _cabi.DlesmError(_cabi.EINVAL, f"{who}: the grid has no message tables (grid_init after decompose)")
    return grid_mod.halo_plan(g)


def invoke_shallow_step_x2_dm(params, u, v, p, uold, vold, pold, unew, vnew, pnew, unew2, vnew2, pnew2, stream=None):
    """TWO leapfrog steps and ONE depth-2 exchange on a decomposed grid (dlesm_shallow_step_x2_dm; halo_width = 2): level n+2
    into unew2.. with valid depth-2 halos, level n+1 into unew.. on the box grown by one cell towards every neighbour, which is
    all the next call reads of it.  Time loop: (cur, old, new1, new2) <- (new2, new1, old, cur) after every call."""
    _shallow_box("dlesm_shallow_step_x2_dm", params, None, _x2_dm_plan(p.grid, "invoke_shallow_step_x2_dm"),
                 (u, v, p, uold, vold, pold, unew, vnew, pnew, unew2, vnew2, pnew2), stream)


def invoke_shallow_step_smooth_x2_dm(params, alpha, u, v, p, uold, vold, pold, unew2, vnew2, pnew2, uold2, vold2, pold2, stream=None):
    """TWO filtered leapfrog steps and ONE depth-2 exchange on a decomposed grid (dlesm_shallow_step_smooth_x2_dm; halo_width = 2):
    level n+2 into unew2.., the filtered level n+1 into uold2.., both with valid depth-2 halos; inputs untouched.  The filtered
    old level must carry valid depth-1 halos.  Time loop: ping-pong (cur, old) <-> (unew2.., uold2..)."""
    _shallow_box("dlesm_shallow_step_smooth_x2_dm", params, alpha, _x2_dm_plan(p.grid, "invoke_shallow_step_smooth_x2_dm"),
                 (u, v, p, uold, vold, pold, unew2, vnew2, pnew2, uold2, vold2, pold2), stream)


def halo_exchange_multi(fields, stream=None, dirs=_cabi.DIRS_ALL):
    """halo_exchange(1) of several fields of one grid in a single grouped RCCL launch"""
    g = fields[0].grid
    arr = (C.c_void_p * len(fields))(*[f.device_ptr.value for f in fields])
    check(_cabi.lib().dlesm_halo_exchange_multi_f64(grid_mod.halo_plan(g), arr, len(fields), dirs,
                                                    _stream_ptr(stream)))


def hash_init(fld, seed, box=None, stream=None):
    """synthetic initial condition on `box` (default: the field's whole region), a function of
    the GLOBAL cell index so that every decomposition produces the same global field"""
    g = fld.grid
    b = box or fld.whole
    s = g.subdomain
    gx0 = s.glob.xstart - s.internal.xstart + 1    # global index of local cell 1
    gy0 = s.glob.ystart - s.internal.ystart + 1
    check(_cabi.lib().dlesm_hash_init_f64(fld.device_ptr, g.nx, g.ny, b.xstart, b.xstop, b.ystart,
                                          b.ystop, seed, gx0, gy0, _stream_ptr(stream)))
