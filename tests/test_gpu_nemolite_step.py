"""GPU tests (-m gpu) of the one-call NEMOLite2D-class time step, dlesm_nemolite_step_f64: bit for bit
the five entries it stands for (continuity -> next_sshu / next_sshv -> fused momentum -> bc_open) on whole arrays -- box, ring
and padding of sentinel-filled outputs, a ring ssha of distinct values the call must read and not write -- with the wave
tile, the definition path (HOOK key nemo_step_kernel, odd pitches, unaligned bases, unequal boxes), with and without an
open-boundary plan; the refusals; a closed basin and a tidal open channel run 30 steps through the one call against the CPU
restatements; and one step at 4096^2."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import momentum_numpy as M
import open_bc_numpy as B
import oracle_lib as O
from nemolite_boxes import INS, METRICS, MOM, OUTS, PRM, _dev, _host_inputs, _host_outputs, _plan, _raw_grid

pytestmark = pytest.mark.gpu


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


def _p(t):
    return C.c_void_p(t.data_ptr())


def _sequence(D, prm, mg, gdev, ld, ny, tbox, ubox, vbox, plan, ssh_bc, I, O_):
    L, ck = D._cabi.lib(), D._cabi.check
    ck(L.dlesm_continuity_f64(prm.rdt, ld, ny, *tbox, *[_p(I[k]) for k in ("sshn_t", "sshn_u", "sshn_v", "hu", "hv", "un", "vn")],
                              _p(gdev["area_t"]), _p(O_["ssha"]), None))
    ck(L.dlesm_next_sshu_f64(ld, ny, *ubox, _p(gdev["tmask"]), _p(gdev["area_t"]), _p(gdev["area_u"]), _p(O_["ssha"]),
                             _p(O_["ssha_u"]), None))
    ck(L.dlesm_next_sshv_f64(ld, ny, *vbox, _p(gdev["tmask"]), _p(gdev["area_t"]), _p(gdev["area_v"]), _p(O_["ssha"]),
                             _p(O_["ssha_v"]), None))
    ck(L.dlesm_momentum_f64(C.byref(prm), C.byref(mg), ld, ny, C.byref(D._cabi.Region(0, 0, *ubox)),
                            C.byref(D._cabi.Region(0, 0, *vbox)), *[_p((I if k in I else O_)[k]) for k in MOM],
                            _p(O_["ua"]), _p(O_["va"]), None))
    if plan is not None:
        ck(L.dlesm_bc_open_f64(plan, C.byref(prm), ssh_bc, *[_p(I[k]) for k in ("hu", "sshn_u", "hv", "sshn_v", "sshn_t")],
                               _p(O_["ssha"]), _p(O_["ua"]), _p(O_["va"]), None))


def _one_call(D, prm, mg, gdev, ld, ny, tbox, ubox, vbox, plan, ssh_bc, I, O_):
    return D._cabi.lib().dlesm_nemolite_step_f64(C.byref(prm), C.byref(mg), _p(gdev["area_t"]), ld, ny,
                                                 C.byref(D._cabi.Region(0, 0, *tbox)), C.byref(D._cabi.Region(0, 0, *ubox)),
                                                 C.byref(D._cabi.Region(0, 0, *vbox)), plan, ssh_bc,
                                                 *[_p(I[k]) for k in INS], *[_p(O_[k]) for k in OUTS], None)


def _check_against_sequence(D, ld, ny, tbox, ubox, vbox, shift, with_plan, seed, kernel=0):
    """the one call against the five entries on raw device arrays; returns the host outputs"""
    import torch
    rng = np.random.default_rng(seed)
    tm = B.repair(rng.choice(np.array([-1, 0, 1, 1, 1], dtype=np.int32), size=(ny, ld)))
    G, gdev, mg = _raw_grid(torch, rng, tm)
    Hi, Ho = _host_inputs(rng, (ny, ld)), _host_outputs(rng, (ny, ld))
    I = _dev(torch, Hi, shift)
    Oseq, Oone = _dev(torch, Ho, shift), _dev(torch, Ho, shift)
    prm = D.psy.momentum_params(*PRM)
    plan = None
    if with_plan:
        plan = _plan(D, tm, tbox, ubox, vbox)
    try:
        _set_tuning(D, nemo_step_kernel=kernel)
        _sequence(D, prm, mg, gdev, ld, ny, tbox, ubox, vbox, plan, 0.0625, I, Oseq)
        assert _one_call(D, prm, mg, gdev, ld, ny, tbox, ubox, vbox, plan, 0.0625, I, Oone) == 0, \
            D._cabi.lib().dlesm_last_error()
        torch.cuda.synchronize()
    finally:
        _set_tuning(D, nemo_step_kernel=0)
        if plan is not None:
            D._cabi.lib().dlesm_obc_destroy(plan)
    got = {k: Oone[k].cpu().numpy() for k in OUTS}
    for k in OUTS:
        assert M.same(got[k], Oseq[k].cpu().numpy()), k
    for k in INS:
        assert M.same(I[k].cpu().numpy(), Hi[k]), k
    # the ring ssha: read, never written
    x0, x1, y0, y1 = tbox
    if x1 >= x0 and y1 >= y0:
        assert M.same(got["ssha"][y1, x0 - 1:x1 + 1], Ho["ssha"][y1, x0 - 1:x1 + 1])       # the north ring row
        assert M.same(got["ssha"][y0 - 1:y1 + 1, x1], Ho["ssha"][y0 - 1:y1 + 1, x1])       # the east ring column
        if (x1 - x0 + 1) * (y1 - y0 + 1) > 50:
            assert (got["ua"] != -7.0).any() and (got["ua"] == -7.0).any()
    return tm, G, Hi, Ho, got


@pytest.mark.parametrize("ld,ny", [(300, 70), (301, 41), (256, 33), (1000, 37), (130, 20), (4100, 9), (6, 5)])
@pytest.mark.parametrize("with_plan", [False, True])
@pytest.mark.parametrize("kernel", [0, 1])
def test_one_call_equals_the_sequence(D, ld, ny, with_plan, kernel):
    """NE boxes (one box B with a one-cell ring), even and odd leading dimensions, random -1/0/1 masks with wet and open ring
    cells, non-uniform metrics, a ring ssha of distinct values: every cell of every array equals the five entries' result.
    kernel = 1: the HOOK key forces the definition path"""
    box = (2, ld - 1, 2, ny - 1)
    tm, G, Hi, Ho, got = _check_against_sequence(D, ld, ny, box, box, box, 0, with_plan, ld * 7 + ny, kernel)
    # and against the CPU restatements, in DESIGN.md section 6.6's order
    W = {k: v.copy() for k, v in Ho.items()}
    O.continuity_slabs(PRM[0], ld, box, Hi["sshn_t"], Hi["sshn_u"], Hi["sshn_v"], Hi["hu"], Hi["hv"], Hi["un"], Hi["vn"],
                       G.area_t, W["ssha"])
    if with_plan:
        B.bc_ssh(box, tm, 0.0625, W["ssha"])
    M.next_sshu(box, tm, G.area_t, G.area_u, W["ssha"], W["ssha_u"])
    M.next_sshv(box, tm, G.area_t, G.area_v, W["ssha"], W["ssha_v"])
    hp = M.params(*PRM)
    M.momentum(hp, G, box, box, *[(Hi if k in Hi else W)[k] for k in MOM], W["ua"], W["va"])
    if with_plan:
        B.flather_u(hp, box, tm, Hi["hu"], Hi["sshn_u"], Hi["sshn_t"], W["ua"])
        B.flather_v(hp, box, tm, Hi["hv"], Hi["sshn_v"], Hi["sshn_t"], W["va"])
    for k in OUTS:
        assert M.same(got[k], W[k]), k
    # the east and north faces of B read the ring's ssha: a wet ring cell beside a wet box cell exists
    x1, y1 = box[1], box[3]
    if ld > 8:
        assert ((tm[1:y1, x1 - 1] > 0) & (tm[1:y1, x1] > 0)).any() and ((tm[y1 - 1, 1:x1] > 0) & (tm[y1, 1:x1] > 0)).any()


@pytest.mark.parametrize("ld,ny,tbox,ubox,vbox,shift", [
    (256, 33, (2, 255, 2, 32), (2, 255, 2, 32), (2, 255, 2, 32), 1),     # bases 8 bytes off a 16-byte boundary
    (300, 70, (37, 250, 5, 60), (37, 250, 5, 60), (37, 250, 5, 60), 0),  # one box away from the origin: the tile
    (300, 70, (37, 250, 5, 60), (40, 298, 2, 69), (2, 299, 9, 50), 0),   # three different boxes: the definition path
    (130, 20, (64, 66, 2, 19), (64, 66, 2, 19), (64, 66, 2, 19), 0),     # a three-column box
    (130, 20, (2, 129, 10, 10), (2, 129, 10, 10), (2, 129, 10, 10), 0),  # a one-row box
    (200, 30, (2, 199, 2, 29), (2, 199, 2, 29), (5, 4, 2, 29), 0),       # an empty V box
    (200, 30, (5, 4, 2, 29), (5, 4, 2, 29), (5, 4, 2, 29), 0),           # all boxes empty
])
@pytest.mark.parametrize("with_plan", [False, True])
def test_other_boxes_and_bases(D, ld, ny, tbox, ubox, vbox, shift, with_plan):
    _check_against_sequence(D, ld, ny, tbox, ubox, vbox, shift, with_plan, ld + 5 * ny + 11 * shift)


def test_the_hook_gives_the_tiles_bits(D):
    """the definition path (nemo_step_kernel = 1) and the wave tile give the same bits"""
    import torch
    ld, ny = 516, 130
    box = (2, ld - 1, 2, ny - 1)
    res = []
    for kernel in (0, 1):
        rng = np.random.default_rng(99)
        tm = B.repair(rng.choice(np.array([-1, 0, 1, 1, 1], dtype=np.int32), size=(ny, ld)))
        G, gdev, mg = _raw_grid(torch, rng, tm)
        I, O_ = _dev(torch, _host_inputs(rng, (ny, ld)), 0), _dev(torch, _host_outputs(rng, (ny, ld)), 0)
        _set_tuning(D, nemo_step_kernel=kernel)
        try:
            assert _one_call(D, D.psy.momentum_params(*PRM), mg, gdev, ld, ny, box, box, box, None, 0.0, I, O_) == 0
            torch.cuda.synchronize()
        finally:
            _set_tuning(D, nemo_step_kernel=0)
        res.append({k: O_[k].cpu().numpy() for k in OUTS})
    for k in OUTS:
        assert M.same(res[0][k], res[1][k]), k


def test_aliasing_is_refused(D):
    """every pair of outputs that overlap, an output overlapping an input, a grid array, area_t or tmask, and a plan made for
    other arrays: DLESM_EINVAL before anything is launched -- nothing is written"""
    import torch
    L = D._cabi.lib()
    ld, ny = 64, 20
    rng = np.random.default_rng(5)
    tm = np.ones((ny, ld), dtype=np.int32)
    G, gdev, mg = _raw_grid(torch, rng, tm)
    box = (2, ld - 1, 2, ny - 1)
    prm = D.psy.momentum_params(*PRM)
    I = {k: torch.full((ny, ld), 1.0, dtype=torch.float64, device="cuda") for k in INS}
    big = torch.full((2 * ny, ld), -7.0, dtype=torch.float64, device="cuda")
    half = big[ny // 2:ny // 2 + ny]

    def fresh():
        return {k: torch.full((ny, ld), -7.0, dtype=torch.float64, device="cuda") for k in OUTS}

    cases = []
    for a in range(5):
        for b in range(a + 1, 5):
            O_ = fresh()
            O_[OUTS[a]], O_[OUTS[b]] = big, half                   # two outputs overlap by half
            cases.append(_one_call(D, prm, mg, gdev, ld, ny, box, box, box, None, 0.0, I, O_))
    for o in OUTS:
        for src in ("un", "sshn_t", "hv"):
            O_ = fresh()
            O_[o] = I[src]                                         # an output is an input
            cases.append(_one_call(D, prm, mg, gdev, ld, ny, box, box, box, None, 0.0, I, O_))
    for o, g in (("ssha", "area_t"), ("ua", "area_u"), ("va", "fcor_v"), ("ssha_u", "dx_t")):
        O_ = fresh()
        O_[o] = gdev[g]                                            # an output is a grid array
        cases.append(_one_call(D, prm, mg, gdev, ld, ny, box, box, box, None, 0.0, I, O_))
    tmd = gdev["tmask"]
    cases_before = len(cases)
    other = _plan(D, np.ones((ny, ld + 2), dtype=np.int32), (2, ld, 2, ny - 1), (2, ld, 2, ny - 1), (2, ld, 2, ny - 1))
    try:
        O_ = fresh()
        cases.append(_one_call(D, prm, mg, gdev, ld, ny, box, box, box, other, 0.0, I, O_))    # a plan for ld + 2
    finally:
        L.dlesm_obc_destroy(other)
    assert cases == [D._cabi.EINVAL] * len(cases), cases
    assert cases_before == 10 + 15 + 4
    torch.cuda.synchronize()
    assert bool((big == -7.0).all())
    assert all(bool((t == 1.0).all()) for t in I.values())
    assert bool((tmd == 1).all())
    # ua over tmask
    O_ = fresh()
    rc = D._cabi.lib().dlesm_nemolite_step_f64(C.byref(prm), C.byref(mg), _p(gdev["area_t"]), ld, ny,
                                               *[C.byref(D._cabi.Region(0, 0, *box))] * 3, None, 0.0,
                                               *[_p(I[k]) for k in INS], _p(O_["ssha"]), _p(O_["ssha_u"]), _p(O_["ssha_v"]),
                                               _p(tmd), _p(O_["va"]), None)
    assert rc == D._cabi.EINVAL and b"tmask" in L.dlesm_last_error()
    torch.cuda.synchronize()
    assert bool((tmd == 1).all())


def _grid(D, nx, ny, alignment, user, dxy=1000.0, ndomains=None):
    if alignment is None:
        os.environ.pop("DL_ESM_ALIGNMENT", None)
    else:
        os.environ["DL_ESM_ALIGNMENT"] = str(alignment)
    g = D.grid_type(D.GO_ARAKAWA_C, (1, 1, 2), D.GO_OFFSET_NE)
    if ndomains is None:
        g.decompose(nx, ny)
    else:
        g.decompose(nx, ny, ndomains=ndomains)
    D.grid_init(g, dxy, dxy, tmask=user)
    os.environ.pop("DL_ESM_ALIGNMENT", None)
    return g


def _fields(D, g, H):
    import torch
    T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
    pts = {"ssha": T, "sshn_t": T, "ht": T, "sshn_u": U, "ssha_u": U, "un": U, "ua": U, "hu": U,
           "sshn_v": V, "ssha_v": V, "vn": V, "va": V, "hv": V}
    F = {}
    for k, a in H.items():
        F[k] = D.r2d_field(g, pts[k])
        F[k].data.copy_(torch.from_numpy(a))
    return F


@pytest.mark.parametrize("nx,ny,alignment", [(300, 70, 64), (300, 70, 1), (257, 129, 64), (257, 129, None), (64, 48, 8),
                                             (1000, 37, 64), (5, 4, None)])
@pytest.mark.parametrize("with_plan", [False, True])
def test_python_wrapper_equals_the_separate_wrappers(D, nx, ny, alignment, with_plan):
    """the Python wrapper on a grid with a -1/0/1 user tmask (wet and open ring cells), non-uniform metrics and a varying
    latitude, DL_ESM_ALIGNMENT 64 (the tile) and 1 (odd pitches: the definition path): every cell of every array equals the
    separate wrappers run in DESIGN.md section 6.7's order"""
    import torch
    rng = np.random.default_rng(nx * 13 + ny)
    user = B.repair(rng.choice(np.array([-1, 0, 1, 1, 1], dtype=np.int32), size=(ny + 2, nx + 2)))
    g = _grid(D, nx, ny, alignment, user)
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
    shape = (g.ny, g.nx)
    H = {**_host_inputs(rng, shape), **_host_outputs(rng, shape)}
    F, F2 = _fields(D, g, H), _fields(D, g, H)
    prm = D.psy.momentum_params(*PRM)
    ssh_bc = D.psy.tide_ssh(0.1, 2.0 * math.pi / 43200.0, 777.0) if with_plan else None
    D.psy.invoke_continuity(F["ssha"], F["sshn_t"], F["sshn_u"], F["sshn_v"], F["hu"], F["hv"], F["un"], F["vn"], prm.rdt)
    D.psy.invoke_next_sshu(F["ssha_u"], F["ssha"])
    D.psy.invoke_next_sshv(F["ssha_v"], F["ssha"])
    D.psy.invoke_momentum(prm, F["ua"], F["va"], *[F[k] for k in MOM])
    if with_plan:
        D.psy.invoke_bc_open(prm, ssh_bc, F["ssha"], F["ua"], F["va"], F["hu"], F["sshn_u"], F["hv"], F["sshn_v"], F["sshn_t"])
    D.psy.invoke_nemolite_step(prm, *[F2[k] for k in OUTS], *[F2[k] for k in INS], ssh_bc=ssh_bc)
    torch.cuda.synchronize()
    for k in H:
        assert M.same(F2[k].get_data(), F[k].get_data()), k
    if with_plan and nx >= 64:
        assert D.psy.open_boundary(g).nt > 0


def test_python_wrapper_refusals(D):
    """no Coriolis parameter: GoceanStop; a decomposed grid: GoceanStop naming the halo exchange; nothing is written"""
    import torch
    nx, ny = 64, 32
    user = np.ones((ny + 2, nx + 2), dtype=np.int32)
    g = _grid(D, nx, ny, 64, user)
    rng = np.random.default_rng(3)
    H = {**_host_inputs(rng, (g.ny, g.nx)), **_host_outputs(rng, (g.ny, g.nx))}
    F = _fields(D, g, H)
    prm = D.psy.momentum_params(*PRM)
    with pytest.raises(D._cabi.GoceanStop, match="Coriolis"):
        D.psy.invoke_nemolite_step(prm, *[F[k] for k in OUTS], *[F[k] for k in INS])
    gd = _grid(D, nx, ny, 64, None, ndomains=2)
    assert gd.decomp.ndomains == 2
    D.psy.coriolis(gd)
    Hd = {**_host_inputs(rng, (gd.ny, gd.nx)), **_host_outputs(rng, (gd.ny, gd.nx))}
    Fd = _fields(D, gd, Hd)
    with pytest.raises(D._cabi.GoceanStop, match="decomposed"):
        D.psy.invoke_nemolite_step(prm, *[Fd[k] for k in OUTS], *[Fd[k] for k in INS], ssh_bc=0.25)
    torch.cuda.synchronize()
    for k in OUTS:
        assert M.same(F[k].get_data(), H[k]) and M.same(Fd[k].get_data(), Hd[k]), k


def _time_loop(D, user, nx, ny, steps, amp, bump):
    import torch
    rdt = PRM[0]
    omega = 2.0 * math.pi / (12.0 * 3600.0)
    g = _grid(D, nx, ny, 64, user)
    D.psy.coriolis(g)
    G = M.SimpleNamespace(tmask=g.tmask_device.cpu().numpy(),
                          **{k: getattr(g, k + "_device").cpu().numpy() for k in METRICS},
                          fcor_u=g.fcor[2].cpu().numpy(), fcor_v=g.fcor[3].cpu().numpy())
    names = ("ssha", "sshn_t", "sshn_u", "sshn_v", "ssha_u", "ssha_v", "un", "vn", "ua", "va", "ht", "hu", "hv")
    H = {k: np.zeros((g.ny, g.nx)) for k in names}
    for k in ("ht", "hu", "hv"):
        H[k][:] = 10.0
    if bump:
        jj, ii = np.mgrid[0:g.ny, 0:g.nx]
        H["sshn_t"][:] = 0.01 * np.exp(-((ii - 0.6 * nx) ** 2 + (jj - 0.5 * ny) ** 2) / (2 * 60.0 ** 2))
    F = _fields(D, g, H)
    tb, ub, vb = F["ssha"].internal.box(), F["ua"].internal.box(), F["va"].internal.box()
    assert tb == ub == vb
    prm, hp = D.psy.momentum_params(*PRM), M.params(*PRM)
    for step in range(steps):
        ssh_bc = None if amp is None else D.psy.tide_ssh(amp, omega, (step + 1) * rdt)
        D.psy.invoke_nemolite_step(prm, *[F[k] for k in OUTS], *[F[k] for k in INS], ssh_bc=ssh_bc)
        O.continuity_slabs(rdt, g.nx, tb, H["sshn_t"], H["sshn_u"], H["sshn_v"], H["hu"], H["hv"], H["un"], H["vn"],
                           G.area_t, H["ssha"])
        if amp is not None:
            B.bc_ssh(tb, G.tmask, B.tide(amp, omega, (step + 1) * rdt), H["ssha"])
        M.next_sshu(ub, G.tmask, G.area_t, G.area_u, H["ssha"], H["ssha_u"])
        M.next_sshv(vb, G.tmask, G.area_t, G.area_v, H["ssha"], H["ssha_v"])
        M.momentum(hp, G, ub, vb, *[H[k] for k in MOM], H["ua"], H["va"])
        if amp is not None:
            B.flather_u(hp, ub, G.tmask, H["hu"], H["sshn_u"], H["sshn_t"], H["ua"])
            B.flather_v(hp, vb, G.tmask, H["hv"], H["sshn_v"], H["sshn_t"], H["va"])
        torch.cuda.synchronize()
        for k in names:
            assert M.same(F[k].get_data(), H[k]), (step, k)
        for a, b in (("un", "ua"), ("vn", "va"), ("sshn_t", "ssha"), ("sshn_u", "ssha_u"), ("sshn_v", "ssha_v")):
            F[a], F[b] = F[b], F[a]
            H[a], H[b] = H[b], H[a]
    for k in names:
        assert np.all(np.isfinite(H[k])), k
    return tb, H


def test_closed_basin_time_loop(D):
    """1024^2, a closed basin with an island and a bump of the surface: 30 steps of the one call, every array bit for bit
    against the continuity oracle + momentum_numpy after every step"""
    n = 1024
    user = np.ones((n + 2, n + 2), dtype=np.int32)
    user[0, :] = user[-1, :] = 0
    user[:, 0] = user[:, -1] = 0
    user[400:520, 300:380] = 0
    _, H = _time_loop(D, user, n, n, 30, None, True)
    assert float(np.abs(H["un"]).max()) > 0.0 and float(np.abs(H["vn"]).max()) > 0.0


def test_open_channel_time_loop(D):
    """1024 x 256, open first and last internal columns, land rows north and south, a tide of period 12 h: 30 steps of the
    one call with ssh_bc, every array bit for bit against open_bc_numpy + momentum_numpy + the continuity oracle"""
    nx, ny = 1024, 256
    user = np.ones((ny + 2, nx + 2), dtype=np.int32)
    user[:, 0] = user[:, -1] = 0
    user[:, 1] = user[:, nx] = -1
    user[:2, :] = 0
    user[-2:, :] = 0
    tb, H = _time_loop(D, user, nx, ny, 30, 0.1, False)
    west = tb[0]                                                # the open west column (1-based)
    assert (H["sshn_t"][1:-1, west] != 0.0).any() and (H["un"][:, west - 1] != 0.0).any()


@pytest.mark.parametrize("with_plan", [False, True])
def test_4096_whole_fields(D, with_plan):
    """one step at 4096^2 (the tile) against the five entries, whole fields"""
    n = 4096
    _check_against_sequence(D, n + 2, n + 2, (2, n + 1, 2, n + 1), (2, n + 1, 2, n + 1), (2, n + 1, 2, n + 1), 0, with_plan,
                            4096)
