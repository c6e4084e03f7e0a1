"""GPU tests (-m gpu) of the open-boundary kernels against the independent CPU restatement
tests/open_bc_numpy.py, bit for bit on whole arrays: the four entries through the Python wrappers on the momentum tests' shape
list, boxes away from the array's origin through the C entries, the fused entry against the separate ones, the aliasing
refusals, a mask with no open cell, the parity of the device's f64 sqrt and division with numpy (correctly rounded) over the
whole double range, and a tidally forced open channel run for 30 steps with continuity and the momentum kernels."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import momentum_numpy as M
import open_bc_numpy as B
import oracle_lib as O

pytestmark = pytest.mark.gpu

PRM = (20.0, 0.00015, 50.0, 9.80665)          # rdt, cbfr, visc, g


@pytest.fixture(scope="module")
def D():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    import dl_esm_inf_amd as d
    torch.cuda.set_device(0)
    d.parallel_init(0, 1)
    return d


def _grid(D, nx, ny, alignment, user, dxy=1000.0):
    if alignment is None:
        os.environ.pop("DL_ESM_ALIGNMENT", None)
    else:
        os.environ["DL_ESM_ALIGNMENT"] = str(alignment)
    g = D.grid_type(D.GO_ARAKAWA_C, (1, 1, 2), D.GO_OFFSET_NE)
    g.decompose(nx, ny)
    D.grid_init(g, dxy, dxy, tmask=user)
    os.environ.pop("DL_ESM_ALIGNMENT", None)
    return g


def _field(D, g, pts, host):
    import torch
    f = D.r2d_field(g, pts)
    f.data.copy_(torch.from_numpy(host))
    return f


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.mark.parametrize("nx,ny,alignment", [(5, 4, None), (64, 48, 8), (300, 70, 64), (257, 129, None), (1, 1, 2),
                                             (129, 3, 2), (1000, 37, 64), (4100, 9, 64)])
def test_four_entries_match_the_checker(D, nx, ny, alignment):
    """the Python wrappers on a grid with a random -1/0/1 user tmask: ssha sentinel-filled, ua / va random; every cell of every
    array equals open_bc_numpy, and bc_open equals bc_ssh + flather_u + flather_v"""
    import torch
    rng = np.random.default_rng(nx * 17 + ny)
    user = B.repair(rng.choice(np.array([-1, 0, 1, 1, 1], dtype=np.int32), size=(ny + 2, nx + 2)))
    g = _grid(D, nx, ny, alignment, user)
    T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
    shape = (g.ny, g.nx)
    tm = g.tmask
    H = {"hu": 1.0 + 20.0 * rng.random(shape), "hv": 1.0 + 20.0 * rng.random(shape),
         "sshn_u": 0.1 * rng.normal(size=shape), "sshn_v": 0.1 * rng.normal(size=shape), "sshn_t": 0.1 * rng.normal(size=shape),
         "ssha": np.full(shape, -7.0), "ua": rng.normal(size=shape), "va": rng.normal(size=shape)}
    pts = {"hu": U, "hv": V, "sshn_u": U, "sshn_v": V, "sshn_t": T, "ssha": T, "ua": U, "va": V}
    F = {k: _field(D, g, pts[k], v) for k, v in H.items()}
    F2 = {k: _field(D, g, pts[k], H[k]) for k in ("ssha", "ua", "va")}
    tb, ub, vb = F["ssha"].internal.box(), F["ua"].internal.box(), F["va"].internal.box()
    assert B.refusal(tm, ub, vb) is None
    prm, hp = D.psy.momentum_params(*PRM), M.params(*PRM)
    ssh_bc = D.psy.tide_ssh(0.1, 2.0 * math.pi / 43200.0, 1234.0)
    assert ssh_bc == B.tide(0.1, 2.0 * math.pi / 43200.0, 1234.0)
    D.psy.invoke_bc_ssh(F["ssha"], ssh_bc)
    D.psy.invoke_bc_flather_u(prm, F["ua"], F["hu"], F["sshn_u"], F["sshn_t"])
    D.psy.invoke_bc_flather_v(prm, F["va"], F["hv"], F["sshn_v"], F["sshn_t"])
    D.psy.invoke_bc_open(prm, ssh_bc, F2["ssha"], F2["ua"], F2["va"], F["hu"], F["sshn_u"], F["hv"], F["sshn_v"], F["sshn_t"])
    torch.cuda.synchronize()
    W = {k: H[k].copy() for k in ("ssha", "ua", "va")}
    B.bc_open(hp, tb, ub, vb, tm, ssh_bc, H["hu"], H["sshn_u"], H["hv"], H["sshn_v"], H["sshn_t"], W["ssha"], W["ua"], W["va"])
    for k in ("ssha", "ua", "va"):
        assert M.same(F[k].get_data(), W[k]), k
        assert M.same(F2[k].get_data(), W[k]), k
    for k in ("hu", "hv", "sshn_u", "sshn_v", "sshn_t"):
        assert M.same(F[k].get_data(), H[k]), k
    plan = D.psy.open_boundary(g)
    assert D.psy.open_boundary(g) is plan
    S = lambda a, b, di=0, dj=0: a[b[2] - 1 + dj:b[3] + dj, b[0] - 1 + di:b[1] + di]   # noqa: E731
    assert plan.nt == int((S(tm, tb) < 0).sum())
    assert plan.nu == int((((S(tm, ub) < 0) & (S(tm, ub, 1) > 0)) | ((S(tm, ub) > 0) & (S(tm, ub, 1) < 0))).sum())
    assert plan.nv == int((((S(tm, vb) < 0) & (S(tm, vb, 0, 1) > 0)) | ((S(tm, vb) > 0) & (S(tm, vb, 0, 1) < 0))).sum())
    if nx >= 64:
        assert plan.nt > 0 and plan.nu > 0 and plan.nv > 0
        assert (W["ua"] != H["ua"]).any() and (W["va"] != H["va"]).any() and (W["ssha"] == ssh_bc).any()
    D.grid_init(g, 1000.0, 1000.0, tmask=np.ones_like(user))        # a new mask: grid_init drops the plan
    assert g._obc is None and D.psy.open_boundary(g).nt == 0


def _plan(D, tm, tbox, ubox, vbox):
    ny, ld = tm.shape
    tm = np.ascontiguousarray(tm, dtype=np.int32)
    h = C.c_void_p()
    D._cabi.check(D._cabi.lib().dlesm_obc_create(tm.ctypes.data, ld, ny, C.byref(D._cabi.Region(0, 0, *tbox)),
                                                 C.byref(D._cabi.Region(0, 0, *ubox)), C.byref(D._cabi.Region(0, 0, *vbox)),
                                                 C.byref(h)))
    return h


@pytest.mark.parametrize("ld,ny,tbox,ubox,vbox", [
    (300, 70, (37, 250, 5, 60), (40, 298, 2, 69), (2, 299, 9, 50)),     # boxes away from the origin, all different
    (301, 41, (1, 301, 1, 41), (2, 300, 3, 40), (9, 17, 2, 38)),        # odd leading dimension; a T box over the whole array
    (130, 20, (64, 66, 2, 19), (2, 129, 10, 10), (5, 4, 2, 19)),        # a three-column box, a one-row box, an empty V box
])
def test_boxes_away_from_the_origin_and_fused_equals_separate(D, ld, ny, tbox, ubox, vbox):
    import torch
    L = D._cabi.lib()
    rng = np.random.default_rng(ld + 3 * ny)
    tm = B.repair(rng.choice(np.array([-1, 0, 1, 1, 1], dtype=np.int32), size=(ny, ld)))
    assert B.refusal(tm, ubox, vbox) is None
    h = _plan(D, tm, tbox, ubox, vbox)
    try:
        host = [1.0 + 20.0 * rng.random((ny, ld)), 0.1 * rng.normal(size=(ny, ld)), 1.0 + 20.0 * rng.random((ny, ld)),
                0.1 * rng.normal(size=(ny, ld)), 0.1 * rng.normal(size=(ny, ld))]          # hu, sshn_u, hv, sshn_v, sshn_t
        outs = [np.full((ny, ld), -7.0), rng.normal(size=(ny, ld)), rng.normal(size=(ny, ld))]   # ssha, ua, va
        dev = [torch.from_numpy(a).cuda() for a in host]
        sep = [torch.from_numpy(a).cuda() for a in outs]
        fus = [torch.from_numpy(a).cuda() for a in outs]
        prm = D.psy.momentum_params(*PRM)
        hu, su, hv, sv, st = (_p(t) for t in dev)
        D._cabi.check(L.dlesm_bc_ssh_f64(h, 0.03125, _p(sep[0]), None))
        D._cabi.check(L.dlesm_bc_flather_u_f64(h, C.byref(prm), hu, su, st, _p(sep[1]), None))
        D._cabi.check(L.dlesm_bc_flather_v_f64(h, C.byref(prm), hv, sv, st, _p(sep[2]), None))
        D._cabi.check(L.dlesm_bc_open_f64(h, C.byref(prm), 0.03125, hu, su, hv, sv, st, *[_p(t) for t in fus], None))
        torch.cuda.synchronize()
        want = [a.copy() for a in outs]
        B.bc_open(M.params(*PRM), tbox, ubox, vbox, tm, 0.03125, *host, *want)
        for k in range(3):
            assert M.same(sep[k].cpu().numpy(), want[k]), k
            assert M.same(fus[k].cpu().numpy(), want[k]), k
        assert (want[0] == 0.03125).any() and (want[1] != outs[1]).any()
    finally:
        L.dlesm_obc_destroy(h)


def test_aliasing_is_refused(D):
    """an output that overlaps an input, or two outputs of the fused entry that overlap, are refused with DLESM_EINVAL and
    nothing is written"""
    import torch
    L = D._cabi.lib()
    ld, ny = 64, 20
    tm = np.ones((ny, ld), dtype=np.int32)
    tm[:, 1] = -1
    tm[1, :] = -1
    tm = B.repair(tm)
    box = (2, ld - 1, 2, ny - 1)
    h = _plan(D, tm, box, box, box)
    try:
        prm = D.psy.momentum_params(*PRM)
        ins = [torch.ones((ny, ld), dtype=torch.float64, device="cuda") for _ in range(5)]
        hu, su, hv, sv, st = (_p(t) for t in ins)
        big = torch.full((2 * ny, ld), -7.0, dtype=torch.float64, device="cuda")
        half = big[ny // 2:ny // 2 + ny]
        a, b = (torch.full((ny, ld), -7.0, dtype=torch.float64, device="cuda") for _ in range(2))
        cases = [
            L.dlesm_bc_flather_u_f64(h, C.byref(prm), hu, su, st, hu, None),                  # ua is hu
            L.dlesm_bc_flather_u_f64(h, C.byref(prm), hu, su, st, st, None),                  # ua is sshn_t
            L.dlesm_bc_flather_v_f64(h, C.byref(prm), _p(big), sv, st, _p(half), None),       # va overlaps hv by half
            L.dlesm_bc_open_f64(h, C.byref(prm), 0.5, hu, su, hv, sv, st, _p(a), _p(a), _p(b), None),       # ssha is ua
            L.dlesm_bc_open_f64(h, C.byref(prm), 0.5, hu, su, hv, sv, st, _p(a), _p(big), _p(half), None),  # ua overlaps va
            L.dlesm_bc_open_f64(h, C.byref(prm), 0.5, hu, su, hv, sv, st, _p(b), _p(a), sv, None),          # va is sshn_v
            L.dlesm_bc_open_f64(h, C.byref(prm), 0.5, hu, su, hv, sv, _p(a), _p(a), _p(b), _p(big), None),  # ssha is sshn_t
        ]
        assert cases == [D._cabi.EINVAL] * len(cases), cases
        torch.cuda.synchronize()
        assert bool((a == -7.0).all()) and bool((b == -7.0).all()) and bool((big == -7.0).all())
        assert all(bool((t == 1.0).all()) for t in ins)
    finally:
        L.dlesm_obc_destroy(h)


def test_a_mask_without_open_cells_leaves_every_array_untouched(D):
    import torch
    rng = np.random.default_rng(11)
    nx, ny = 200, 60
    user = np.ones((ny + 2, nx + 2), dtype=np.int32)
    user[:, :40] = 0
    g = _grid(D, nx, ny, 64, user)
    plan = D.psy.open_boundary(g)
    assert (plan.nt, plan.nu, plan.nv) == (0, 0, 0)
    shape = (g.ny, g.nx)
    T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
    H = [rng.normal(size=shape) for _ in range(8)]
    F = [_field(D, g, p, a) for p, a in zip((U, U, V, V, T, T, U, V), H)]
    prm = D.psy.momentum_params(*PRM)
    D.psy.invoke_bc_ssh(F[5], 0.25)
    D.psy.invoke_bc_flather_u(prm, F[6], F[0], F[1], F[4])
    D.psy.invoke_bc_flather_v(prm, F[7], F[2], F[3], F[4])
    D.psy.invoke_bc_open(prm, 0.25, F[5], F[6], F[7], *F[:5])
    torch.cuda.synchronize()
    for f, a in zip(F, H):
        assert M.same(f.get_data(), a)


def _parity_depths(rng, n):
    """depths from 1e-300 to 1e300 with random mantissas, exact powers of four, 1/k^2, subnormal and zero depths, and a few
    negative ones (sqrt of a negative number: NaN)"""
    e = rng.uniform(-300.0, 300.0, n)
    h = (1.0 + rng.random(n)) * 10.0 ** np.floor(e)
    k = rng.integers(0, n, n // 8)
    h[k] = np.ldexp(1.0, 2 * rng.integers(-500, 500, k.size))                        # g/h an exact square when g is one
    k = rng.integers(0, n, n // 8)
    h[k] = 1.0 / (rng.integers(1, 1 << 26, k.size).astype(np.float64) ** 2)
    h[rng.integers(0, n, n // 64)] = 0.0
    h[rng.integers(0, n, n // 64)] = 5e-324 * rng.integers(1, 1 << 40, n // 64)          # subnormal depths
    h[rng.integers(0, n, n // 256)] *= -1.0
    return h


@pytest.mark.parametrize("g", [9.80665, 1.0, 1e-10, 3.0e-300])
def test_sqrt_parity_with_numpy(D, g):
    """c = sqrt(g/h) over the whole double range, bit for bit numpy's correctly rounded division and sqrt (NaN equal to NaN).
    With ua = sshn_u = 0 and sshn_t = 1 every written u / v cell is exactly -c*(0-1) = c (open side west / south) or
    +c*(0-1) = -c (east / north), so each one shows the device's c itself.  g/h is subnormal for g = 1e-10 and h > 1e298, and
    for g = 3e-300; h = 0 gives c = inf."""
    import torch
    L = D._cabi.lib()
    ld, ny = 1028, 258
    tm = np.tile(np.array([-1, 1, 1, -1], dtype=np.int32), (ny, ld // 4))
    tm[2::4, :] = -1                                           # open rows: open v faces to the south and to the north
    tm = B.repair(tm)
    box = (2, ld - 1, 2, ny - 1)
    assert B.refusal(tm, box, box) is None
    h = _plan(D, tm, box, box, box)
    try:
        nt, nu, nv = C.c_int(), C.c_int(), C.c_int()
        L.dlesm_obc_counts(h, C.byref(nt), C.byref(nu), C.byref(nv))
        assert nu.value > 50000 and nv.value > 20000
        rng = np.random.default_rng(int(-math.log10(g) * 10) + 400)
        hu, hv = _parity_depths(rng, ld * ny).reshape(ny, ld), _parity_depths(rng, ld * ny).reshape(ny, ld)
        zero, one = np.zeros((ny, ld)), np.ones((ny, ld))
        dev = [torch.from_numpy(a.copy()).cuda() for a in (hu, zero, hv, zero, one, zero, zero)]
        prm = D.psy.momentum_params(20.0, 0.0, 0.0, g)
        D._cabi.check(L.dlesm_bc_flather_u_f64(h, C.byref(prm), *[_p(t) for t in (dev[0], dev[1], dev[4], dev[5])], None))
        D._cabi.check(L.dlesm_bc_flather_v_f64(h, C.byref(prm), *[_p(t) for t in (dev[2], dev[3], dev[4], dev[6])], None))
        torch.cuda.synchronize()
        hp = M.params(20.0, 0.0, 0.0, g)
        for k, (hh, fn) in enumerate(((hu, B.flather_u), (hv, B.flather_v))):
            want = np.zeros((ny, ld))
            fn(hp, box, tm, hh, zero, one, want)
            got = dev[5 + k].cpu().numpy()
            di, dj = (1, 0) if k == 0 else (0, 1)
            written = np.zeros((ny, ld), dtype=bool)
            t0, t1 = tm[1:ny - 1, 1:ld - 1], tm[1 + dj:ny - 1 + dj, 1 + di:ld - 1 + di]
            written[1:ny - 1, 1:ld - 1] = ((t0 < 0) & (t1 > 0)) | ((t0 > 0) & (t1 < 0))
            assert written.sum() == (nu.value if k == 0 else nv.value)
            with np.errstate(all="ignore"):
                c = np.sqrt(g / hh)
            assert M.same(np.abs(want[written]), np.abs(c[written]))       # the restatement's c is numpy's
            if g < 1e-9:
                with np.errstate(all="ignore"):
                    q = g / hh[written]
                assert ((q > 0) & (q < 2.2250738585072014e-308)).any()    # subnormal quotients among the written cells
            bad = ~((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want)))
            assert not bad.any(), (k, int(bad.sum()), hh[bad][:5], got[bad][:5], want[bad][:5])
    finally:
        L.dlesm_obc_destroy(h)


@pytest.mark.parametrize("amp", [0.0, 0.1])
def test_open_channel_time_loop(D, amp):
    """1024 x 256, depth 10 m, dx = 1 km, rdt = 20 s: open (-1) first and last internal columns, land rows north and south, a
    tide of period 12 h.  30 steps of continuity -> next_sshu / next_sshv -> fused momentum -> bc_open (the fused boundary entry
    after momentum: next_ssh* never read an open cell's ssha, so this is DESIGN.md section 6.6's order), rotating by reference;
    every array bit for bit against open_bc_numpy + momentum_numpy + the continuity oracle, evaluated in section 6.6's order,
    after every step.  amp = 0: the state at rest stays exactly 0.  amp > 0: the tide comes in at the west boundary and
    columns further than 4 x steps from both boundaries stay exactly 0."""
    import torch
    nx, ny, steps, rdt = 1024, 256, 30, 20.0
    omega = 2.0 * math.pi / (12.0 * 3600.0)
    user = np.ones((ny + 2, nx + 2), dtype=np.int32)
    user[:, 0] = user[:, -1] = 0
    user[:, 1] = user[:, nx] = -1
    user[:2, :] = 0
    user[-2:, :] = 0
    g = _grid(D, nx, ny, 64, user)
    D.psy.coriolis(g)
    G = M.SimpleNamespace(tmask=g.tmask_device.cpu().numpy(),
                          **{k: getattr(g, k + "_device").cpu().numpy() for k in ("dx_t", "dy_t", "dx_u", "dy_u", "dx_v",
                                                                                  "dy_v", "area_u", "area_v")},
                          fcor_u=g.fcor[2].cpu().numpy(), fcor_v=g.fcor[3].cpu().numpy())
    area_t = g.area_t_device.cpu().numpy()
    T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
    names = ("ssha", "sshn_t", "sshn_u", "sshn_v", "ssha_u", "ssha_v", "un", "vn", "ua", "va", "ht", "hu", "hv")
    pts = (T, T, U, V, U, V, U, V, U, V, T, U, V)
    H = {k: np.zeros((g.ny, g.nx)) for k in names}
    for k in ("ht", "hu", "hv"):
        H[k][:] = 10.0
    F = {k: _field(D, g, p, H[k]) for k, p in zip(names, pts)}
    plan = D.psy.open_boundary(g)
    assert (plan.nt, plan.nu, plan.nv) == (2 * (ny - 2), 2 * (ny - 2), 0)
    prm, hp = D.psy.momentum_params(rdt, 0.00015, 50.0, 9.80665), M.params(rdt, 0.00015, 50.0, 9.80665)
    tb, ub, vb = F["ssha"].internal.box(), F["ua"].internal.box(), F["va"].internal.box()
    west, east = tb[0], tb[1]                                   # the open columns (1-based)
    mom = ("un", "vn", "ht", "sshn_t", "hu", "sshn_u", "hv", "sshn_v", "ssha_u", "ssha_v")
    for step in range(steps):
        ssh_bc = D.psy.tide_ssh(amp, omega, (step + 1) * rdt)
        D.psy.invoke_continuity(F["ssha"], F["sshn_t"], F["sshn_u"], F["sshn_v"], F["hu"], F["hv"], F["un"], F["vn"], rdt)
        D.psy.invoke_next_sshu(F["ssha_u"], F["ssha"])
        D.psy.invoke_next_sshv(F["ssha_v"], F["ssha"])
        D.psy.invoke_momentum(prm, F["ua"], F["va"], *[F[k] for k in mom])
        D.psy.invoke_bc_open(prm, ssh_bc, F["ssha"], F["ua"], F["va"], F["hu"], F["sshn_u"], F["hv"], F["sshn_v"], F["sshn_t"])
        O.continuity_slabs(rdt, g.nx, tb, H["sshn_t"], H["sshn_u"], H["sshn_v"], H["hu"], H["hv"], H["un"], H["vn"], area_t,
                           H["ssha"])
        B.bc_ssh(tb, G.tmask, B.tide(amp, omega, (step + 1) * rdt), H["ssha"])
        M.next_sshu(ub, G.tmask, area_t, G.area_u, H["ssha"], H["ssha_u"])
        M.next_sshv(vb, G.tmask, area_t, G.area_v, H["ssha"], H["ssha_v"])
        M.momentum(hp, G, ub, vb, *[H[k] for k in mom], H["ua"], H["va"])
        B.flather_u(hp, ub, G.tmask, H["hu"], H["sshn_u"], H["sshn_t"], H["ua"])
        B.flather_v(hp, vb, G.tmask, H["hv"], H["sshn_v"], H["sshn_t"], H["va"])
        torch.cuda.synchronize()
        for k in names:
            assert M.same(F[k].get_data(), H[k]), (step, k)
        for a, b in (("un", "ua"), ("vn", "va"), ("sshn_t", "ssha"), ("sshn_u", "ssha_u"), ("sshn_v", "ssha_v")):
            F[a], F[b] = F[b], F[a]
            H[a], H[b] = H[b], H[a]
        reach = 4 * (step + 1)
        for k in names[:10]:
            if amp == 0.0:
                assert not H[k].any(), (step, k)
            else:
                assert not H[k][:, west - 1 + reach + 1:east - reach - 1].any(), (step, k)
    for k in names:
        assert np.all(np.isfinite(H[k])), k
    if amp > 0.0:
        assert (H["sshn_t"][1:-1, west] != 0.0).any()           # the cell beside the west boundary has felt the tide
        assert (H["un"][:, west - 1] != 0.0).any()              # and the open face carries a velocity
