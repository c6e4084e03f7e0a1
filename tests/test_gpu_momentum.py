"""GPU tests (-m gpu) of the NEMOLite2D-class momentum and next_ssh kernels against the independent
CPU restatement tests/momentum_numpy.py, bit for bit on whole arrays: box, ring and padding of sentinel-filled outputs.
Both forms of every entry (the wave tile and the one-cell-per-thread form, HOOK key mom_kernel), boxes away from the
array's origin, the fused entry against the separate ones, the aliasing refusals, a 4096^2 fused sweep, the Python
wrappers with their Coriolis refusal, and a closed-basin time loop with the continuity kernel."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import momentum_numpy as M
import oracle_lib as O

pytestmark = pytest.mark.gpu

PRM = (20.0, 0.00015, 50.0, 9.80665)          # rdt, cbfr, visc, g
METRICS = ("dx_t", "dy_t", "dx_u", "dy_u", "dx_v", "dy_v", "area_t", "area_u", "area_v")


@pytest.fixture(scope="module")
def D():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    import dl_esm_inf_amd as d
    torch.cuda.set_device(0)
    d.parallel_init(0, 1)
    return d


def _set_tuning(D, **kw):
    for k, v in kw.items():
        D._cabi.lib().dlesm_set_tuning(k.encode(), v)


def _masked_grid(D, nx, ny, alignment, rng, dxy=1000.0, user=None):
    if alignment is None:
        os.environ.pop("DL_ESM_ALIGNMENT", None)
    else:
        os.environ["DL_ESM_ALIGNMENT"] = str(alignment)
    g = D.grid_type(D.GO_ARAKAWA_C, (1, 1, 2), D.GO_OFFSET_NE)
    g.decompose(nx, ny)
    if user is None:
        user = rng.integers(-1, 2, (ny + 2, nx + 2)).astype(np.int32)
        user[: (ny + 2) // 3, : (nx + 2) // 3] = 0                  # a stretch of coast
    D.grid_init(g, dxy, dxy, tmask=user)
    os.environ.pop("DL_ESM_ALIGNMENT", None)
    return g


def _nonuniform(g, rng):
    """non-uniform metrics on the grid's device mirrors (zero spacings on land: dry cells divide by zero), a latitude that
    varies, and the Coriolis parameter from it"""
    import torch
    import dl_esm_inf_amd as D
    land = g.tmask <= 0
    for name in METRICS:
        a = 900.0 + 200.0 * rng.random((g.ny, g.nx))
        if name.startswith("area"):
            a *= 1000.0
        elif name.endswith("_t"):
            a[land] = 0.0
        getattr(g, name + "_device").copy_(torch.from_numpy(a))
    g.gphiu = 40.0 + 20.0 * rng.random((g.ny, g.nx))
    g.gphiv = 40.0 + 20.0 * rng.random((g.ny, g.nx))
    D.psy.coriolis(g)
    torch.cuda.synchronize()


def _host_grid(g):
    arrs = {name: getattr(g, name + "_device").cpu().numpy() for name in METRICS}
    arrs["fcor_u"], arrs["fcor_v"] = g.fcor[2].cpu().numpy(), g.fcor[3].cpu().numpy()
    return M.SimpleNamespace(tmask=g.tmask_device.cpu().numpy(), **arrs)


def _vel(rng, shape):
    v = rng.normal(0.0, 0.3, shape)
    pick = rng.random(shape)
    v[pick < 0.15] = 0.0
    v[(pick >= 0.15) & (pick < 0.3)] = -0.0
    return v


def _inputs(D, g, rng):
    """un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, ssha_v as fields, and their host copies"""
    import torch
    pts = [D.GO_U_POINTS, D.GO_V_POINTS, D.GO_T_POINTS, D.GO_T_POINTS, D.GO_U_POINTS, D.GO_U_POINTS, D.GO_V_POINTS,
           D.GO_V_POINTS, D.GO_U_POINTS, D.GO_V_POINTS]
    shape = (g.ny, g.nx)
    host = [_vel(rng, shape), _vel(rng, shape)]
    for k in range(2, 10):
        host.append(10.0 + rng.random(shape) if k in (2, 4, 6) else 0.1 * rng.normal(size=shape))
    F = []
    for p, h in zip(pts, host):
        f = D.r2d_field(g, p)
        f.data.copy_(torch.from_numpy(h))
        F.append(f)
    return F, host


def _sentinel(D, g, pts, val=-7.0):
    f = D.r2d_field(g, pts)
    D.set_field(f, val)
    return f


@pytest.mark.parametrize("nx,ny,alignment", [(5, 4, None), (64, 48, 8), (300, 70, 64), (257, 129, None), (1, 1, 2),
                                             (129, 3, 2), (1000, 37, 64), (4100, 9, 64)])
@pytest.mark.parametrize("kernel", [0, 1])
def test_five_entries_match_the_checker(D, nx, ny, alignment, kernel):
    """the Python wrappers of all five entries on a grid with a -1/0/1 user tmask, non-uniform metrics and a varying
    latitude: every cell of every sentinel-filled output equals momentum_numpy"""
    import torch
    _set_tuning(D, mom_kernel=kernel)
    try:
        rng = np.random.default_rng(nx * 31 + ny)
        g = _masked_grid(D, nx, ny, alignment, rng)
        _nonuniform(g, rng)
        F, H = _inputs(D, g, rng)
        G = _host_grid(g)
        prm = D.psy.momentum_params(*PRM)
        hp = M.params(*PRM)
        ua, va, ua2, va2 = (_sentinel(D, g, p) for p in (D.GO_U_POINTS, D.GO_V_POINTS, D.GO_U_POINTS, D.GO_V_POINTS))
        su, sv = _sentinel(D, g, D.GO_U_POINTS), _sentinel(D, g, D.GO_V_POINTS)
        D.psy.invoke_momentum_u(prm, ua, *F[:9])
        D.psy.invoke_momentum_v(prm, va, *F[:8], F[9])
        D.psy.invoke_momentum(prm, ua2, va2, *F)
        D.psy.invoke_next_sshu(su, F[3])
        D.psy.invoke_next_sshv(sv, F[3])
        torch.cuda.synchronize()
        ub, vb = ua.internal.box(), va.internal.box()
        want_u, want_v = np.full((g.ny, g.nx), -7.0), np.full((g.ny, g.nx), -7.0)
        M.momentum_u(hp, G, ub, *H[:9], want_u)
        M.momentum_v(hp, G, vb, *H[:8], H[9], want_v)
        assert M.same(ua.get_data(), want_u) and M.same(ua2.get_data(), want_u)
        assert M.same(va.get_data(), want_v) and M.same(va2.get_data(), want_v)
        for fld, fn, area, box in ((su, M.next_sshu, G.area_u, ub), (sv, M.next_sshv, G.area_v, vb)):
            want = np.full((g.ny, g.nx), -7.0)
            fn(box, G.tmask, G.area_t, area, H[3], want)
            assert M.same(fld.get_data(), want)
        if ub[1] >= ub[0] and nx > 8:
            assert (want_u != -7.0).any() and (want_u == -7.0).any()      # wet and dry faces both present
    finally:
        _set_tuning(D, mom_kernel=0)


def _raw(torch, rng, ny, ld, n):
    """n (ny, ld) device arrays of plausible inputs (velocities first two) and the host copies"""
    host = [_vel(rng, (ny, ld)), _vel(rng, (ny, ld))] + [10.0 + rng.random((ny, ld)) if k % 2 == 0 else 0.1 * rng.normal(size=(ny, ld))
                                                         for k in range(n - 2)]
    return host, [torch.from_numpy(h).cuda() for h in host]


def _raw_grid(torch, rng, ny, ld):
    tm = rng.integers(-1, 2, (ny, ld)).astype(np.int32)
    G = {"tmask": tm}
    for name in M.GRID_ARRAYS[1:9]:
        G[name] = 900.0 + 200.0 * rng.random((ny, ld)) * (1000.0 if name.startswith("area") else 1.0)
    G["fcor_u"] = M.coriolis(40.0 + 20.0 * rng.random((ny, ld)), 7.292116e-5, math.pi / 180.0)
    G["fcor_v"] = M.coriolis(40.0 + 20.0 * rng.random((ny, ld)), 7.292116e-5, math.pi / 180.0)
    dev = {k: torch.from_numpy(v).cuda() for k, v in G.items()}
    from dl_esm_inf_amd import _cabi
    mg = _cabi.MomentumGrid(**{k: dev[k].data_ptr() for k in M.GRID_ARRAYS})
    return M.SimpleNamespace(**G), dev, mg


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("ld,ny,ubox,vbox,shift", [
    (300, 70, (37, 250, 5, 60), (40, 299, 2, 69), 0),       # boxes away from the origin, different U and V boxes
    (301, 41, (2, 300, 3, 40), (9, 17, 2, 38), 0),          # odd leading dimension: the one-cell form
    (256, 33, (3, 255, 2, 32), (2, 200, 4, 30), 1),         # bases 8 bytes off a 16-byte boundary: the one-cell form
    (130, 20, (64, 66, 2, 19), (2, 129, 10, 10), 0),        # a three-column box, a one-row box
    (200, 30, (2, 199, 2, 29), (5, 4, 2, 29), 0),           # an empty V box
])
@pytest.mark.parametrize("kernel", [0, 1])
def test_boxes_away_from_the_origin_and_fused_equals_separate(D, ld, ny, ubox, vbox, shift, kernel):
    import torch
    L = D._cabi.lib()
    _set_tuning(D, mom_kernel=kernel)
    try:
        rng = np.random.default_rng(ld + 7 * ny)
        G, gdev, mg = _raw_grid(torch, rng, ny, ld)
        H, Dv = _raw(torch, rng, ny, ld, 10)
        if shift:
            Dv = [torch.cat([torch.zeros(1, dtype=torch.float64, device="cuda"), t.flatten()])[1:].view(ny, ld) for t in Dv]
            assert Dv[0].data_ptr() % 16 == 8
        outs = [torch.full((ny, ld), -7.0, dtype=torch.float64, device="cuda") for _ in range(4)]
        if shift:
            outs = [torch.cat([torch.zeros(1, dtype=torch.float64, device="cuda"), t.flatten()])[1:].view(ny, ld) for t in outs]
        prm = D.psy.momentum_params(*PRM)
        ins = [_p(t) for t in Dv]
        D._cabi.check(L.dlesm_momentum_u_f64(C.byref(prm), C.byref(mg), ld, ny, *ubox, *ins[:9], _p(outs[0]), None))
        D._cabi.check(L.dlesm_momentum_v_f64(C.byref(prm), C.byref(mg), ld, ny, *vbox, *ins[:8], ins[9], _p(outs[1]), None))
        ur, vr = D._cabi.Region(0, 0, *ubox), D._cabi.Region(0, 0, *vbox)
        D._cabi.check(L.dlesm_momentum_f64(C.byref(prm), C.byref(mg), ld, ny, C.byref(ur), C.byref(vr), *ins, _p(outs[2]),
                                           _p(outs[3]), None))
        torch.cuda.synchronize()
        got = [t.cpu().numpy() for t in outs]
        assert M.same(got[0], got[2]) and M.same(got[1], got[3])
        hp = M.params(*PRM)
        want_u, want_v = np.full((ny, ld), -7.0), np.full((ny, ld), -7.0)
        M.momentum_u(hp, G, ubox, *H[:9], want_u)
        M.momentum_v(hp, G, vbox, *H[:8], H[9], want_v)
        assert M.same(got[0], want_u) and M.same(got[1], want_v)
        for fn, cfn, area, box in ((M.next_sshu, L.dlesm_next_sshu_f64, "area_u", ubox), (M.next_sshv, L.dlesm_next_sshv_f64, "area_v", vbox)):
            o = torch.full((ny, ld), -7.0, dtype=torch.float64, device="cuda")
            D._cabi.check(cfn(ld, ny, *box, _p(gdev["tmask"]), _p(gdev["dx_t"]), _p(gdev[area]), ins[3], _p(o), None))
            want = np.full((ny, ld), -7.0)
            fn(box, G.tmask, G.dx_t, getattr(G, area), H[3], want)
            assert M.same(o.cpu().numpy(), want)
    finally:
        _set_tuning(D, mom_kernel=0)


def test_aliasing_is_refused(D):
    """an output that overlaps any input, or ua overlapping va, is refused with DLESM_EINVAL and nothing is written"""
    import torch
    L = D._cabi.lib()
    ld, ny = 64, 20
    rng = np.random.default_rng(5)
    G, gdev, mg = _raw_grid(torch, rng, ny, ld)
    _, Dv = _raw(torch, rng, ny, ld, 10)
    prm = D.psy.momentum_params(*PRM)
    box = (2, ld - 1, 2, ny - 1)
    r = D._cabi.Region(0, 0, *box)
    ua, va = (torch.full((ny, ld), -7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    ins = [_p(t) for t in Dv]
    big = torch.full((2 * ny, ld), -7.0, dtype=torch.float64, device="cuda")
    half = big[ny // 2:ny // 2 + ny]                               # overlaps `big`'s first ny rows by half
    cases = [
        L.dlesm_momentum_u_f64(C.byref(prm), C.byref(mg), ld, ny, *box, *ins[:9], ins[0], None),          # ua is un
        L.dlesm_momentum_u_f64(C.byref(prm), C.byref(mg), ld, ny, *box, *ins[:8], ins[8], ins[8], None),  # ua is ssha_u
        L.dlesm_momentum_v_f64(C.byref(prm), C.byref(mg), ld, ny, *box, *ins[:8], ins[9], _p(gdev["dx_v"]), None),
        L.dlesm_momentum_f64(C.byref(prm), C.byref(mg), ld, ny, C.byref(r), C.byref(r), *ins, _p(ua), _p(ua), None),
        L.dlesm_momentum_f64(C.byref(prm), C.byref(mg), ld, ny, C.byref(r), C.byref(r), *ins[:9], _p(big), _p(ua), _p(half), None),
        L.dlesm_momentum_f64(C.byref(prm), C.byref(mg), ld, ny, C.byref(r), C.byref(r), *ins, _p(big), _p(half), None),
        L.dlesm_next_sshu_f64(ld, ny, *box, _p(gdev["tmask"]), _p(gdev["dx_t"]), _p(gdev["area_u"]), ins[3], ins[3], None),
        L.dlesm_next_sshv_f64(ld, ny, *box, _p(gdev["tmask"]), _p(gdev["dx_t"]), _p(gdev["area_v"]), ins[3], _p(gdev["area_v"]), None),
    ]
    assert cases == [D._cabi.EINVAL] * len(cases), cases
    torch.cuda.synchronize()
    assert bool((ua == -7.0).all()) and bool((big == -7.0).all())


def test_coriolis_once_per_grid_and_the_refusal(D):
    """a momentum wrapper on a grid whose Coriolis parameter was never set stops; psy.coriolis computes it on the host from
    gphiu / gphiv (50 degrees after grid_init: the reference's f-plane) and caches it per grid"""
    import torch
    rng = np.random.default_rng(3)
    g = _masked_grid(D, 40, 30, 8, rng)
    F, _ = _inputs(D, g, rng)
    prm = D.psy.momentum_params(*PRM)
    ua, va = _sentinel(D, g, D.GO_U_POINTS), _sentinel(D, g, D.GO_V_POINTS)
    with pytest.raises(D.GoceanStop, match="Coriolis"):
        D.psy.invoke_momentum_u(prm, ua, *F[:9])
    with pytest.raises(D.GoceanStop, match="Coriolis"):
        D.psy.invoke_momentum_v(prm, va, *F[:8], F[9])
    with pytest.raises(D.GoceanStop, match="Coriolis"):
        D.psy.invoke_momentum(prm, ua, va, *F)
    torch.cuda.synchronize()
    assert bool((ua.data == -7.0).all()) and bool((va.data == -7.0).all())
    assert np.all(g.gphiu == 50.0) and np.all(g.gphiv == 50.0)
    fu, fv = D.psy.coriolis(g)
    f50 = (2.0 * 7.292116e-5) * math.sin(50.0 * (math.pi / 180.0))
    assert np.allclose(fu.cpu().numpy(), f50, rtol=4e-16, atol=0) and np.allclose(fv.cpu().numpy(), f50, rtol=4e-16, atol=0)
    again = D.psy.coriolis(g)
    assert again[0] is fu and again[1] is fv
    D.psy.invoke_momentum(prm, ua, va, *F)
    torch.cuda.synchronize()
    assert bool((ua.data != -7.0).any())


def test_fused_entry_at_4096(D):
    """4096^2, alignment 64, a -1/0/1 mask: every cell of both sentinel-filled outputs of the fused entry"""
    import torch
    n = 4096
    rng = np.random.default_rng(n)
    user = rng.integers(-1, 2, (n + 2, n + 2), dtype=np.int32)
    user[100:900, 200:1500] = 0                                 # land
    g = _masked_grid(D, n, n, 64, rng, user=user)
    del user
    _nonuniform(g, rng)
    F, H = _inputs(D, g, rng)
    G = _host_grid(g)
    ua, va = _sentinel(D, g, D.GO_U_POINTS), _sentinel(D, g, D.GO_V_POINTS)
    D.psy.invoke_momentum(D.psy.momentum_params(*PRM), ua, va, *F)
    torch.cuda.synchronize()
    want_u, want_v = np.full((g.ny, g.nx), -7.0), np.full((g.ny, g.nx), -7.0)
    M.momentum(M.params(*PRM), G, ua.internal.box(), va.internal.box(), *H, want_u, want_v)
    assert M.same(ua.get_data(), want_u)
    assert M.same(va.get_data(), want_v)


def test_closed_basin_time_loop(D):
    """1024^2, a closed basin with an island, depth 10 m, dx = 1 km, rdt = 20 s, a small bump of the surface: 30 steps of
    continuity -> next_sshu / next_sshv -> fused momentum, rotating by reference; every array bit for bit against
    momentum_numpy + the continuity oracle after every step, every value finite"""
    import torch
    n, steps, rdt = 1024, 30, 20.0
    user = np.ones((n + 2, n + 2), dtype=np.int32)
    user[0, :] = user[-1, :] = 0
    user[:, 0] = user[:, -1] = 0
    user[400:520, 300:380] = 0                                   # an island
    g = _masked_grid(D, n, n, 64, None, dxy=1000.0, user=user)
    D.psy.coriolis(g)
    G = _host_grid(g)
    area_t = g.area_t_device.cpu().numpy()
    T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
    names = ("ssha", "sshn_t", "sshn_u", "sshn_v", "ssha_u", "ssha_v", "un", "vn", "ua", "va", "ht", "hu", "hv")
    pts = (T, T, U, V, U, V, U, V, U, V, T, U, V)
    F = {k: D.r2d_field(g, p) for k, p in zip(names, pts)}
    H = {k: np.zeros((g.ny, g.nx)) for k in names}
    for k in ("ht", "hu", "hv"):
        H[k][:] = 10.0
    jj, ii = np.mgrid[0:g.ny, 0:g.nx]
    H["sshn_t"][:] = 0.01 * np.exp(-((ii - 600.0) ** 2 + (jj - 500.0) ** 2) / (2 * 60.0 ** 2))
    for k in names:
        F[k].data.copy_(torch.from_numpy(H[k]))
    D.psy.invoke_next_sshu(F["sshn_u"], F["sshn_t"])
    D.psy.invoke_next_sshv(F["sshn_v"], F["sshn_t"])
    M.next_sshu(F["sshn_u"].internal.box(), G.tmask, area_t, G.area_u, H["sshn_t"], H["sshn_u"])
    M.next_sshv(F["sshn_v"].internal.box(), G.tmask, area_t, G.area_v, H["sshn_t"], H["sshn_v"])
    prm, hp = D.psy.momentum_params(rdt, 0.00015, 50.0, 9.80665), M.params(rdt, 0.00015, 50.0, 9.80665)
    tb, ub, vb = F["ssha"].internal.box(), F["ua"].internal.box(), F["va"].internal.box()
    for step in range(steps):
        D.psy.invoke_continuity(F["ssha"], F["sshn_t"], F["sshn_u"], F["sshn_v"], F["hu"], F["hv"], F["un"], F["vn"], rdt)
        D.psy.invoke_next_sshu(F["ssha_u"], F["ssha"])
        D.psy.invoke_next_sshv(F["ssha_v"], F["ssha"])
        D.psy.invoke_momentum(prm, F["ua"], F["va"], *[F[k] for k in ("un", "vn", "ht", "sshn_t", "hu", "sshn_u", "hv", "sshn_v",
                                                                      "ssha_u", "ssha_v")])
        O.continuity_slabs(rdt, g.nx, tb, H["sshn_t"], H["sshn_u"], H["sshn_v"], H["hu"], H["hv"], H["un"], H["vn"], area_t,
                           H["ssha"])
        M.next_sshu(ub, G.tmask, area_t, G.area_u, H["ssha"], H["ssha_u"])
        M.next_sshv(vb, G.tmask, area_t, G.area_v, H["ssha"], H["ssha_v"])
        M.momentum(hp, G, ub, vb, *[H[k] for k in ("un", "vn", "ht", "sshn_t", "hu", "sshn_u", "hv", "sshn_v", "ssha_u",
                                                   "ssha_v")], H["ua"], H["va"])
        torch.cuda.synchronize()
        for k in names:
            assert M.same(F[k].get_data(), H[k]), (step, k)
        for a, b in (("un", "ua"), ("vn", "va"), ("sshn_t", "ssha"), ("sshn_u", "ssha_u"), ("sshn_v", "ssha_v")):
            F[a], F[b] = F[b], F[a]
            H[a], H[b] = H[b], H[a]
    for k in names:
        assert np.all(np.isfinite(H[k])), k
    assert float(np.abs(H["un"]).max()) > 0.0 and float(np.abs(H["vn"]).max()) > 0.0     # the bump has set the basin moving
