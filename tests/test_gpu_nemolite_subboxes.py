"""GPU tests (-m gpu) of the NEMOLite2D-class kernels on boxes whose edges fall where the wave tiles branch, and on random
boxes of random arrays (tests/nemolite_boxes.py): momentum_u / momentum_v / the fused momentum entry (tile and one-cell
form), next_sshu / next_sshv, the open boundary, and the one-call step (tile and definition path), every cell of every
array against the CPU restatements (tests/momentum_numpy.py, tests/open_bc_numpy.py, the continuity oracle) -- box, ring
and padding of sentinel-filled outputs, a ring ssha of distinct values.  Then IEEE special values through momentum and
the step."""
import ctypes as C

import numpy as np
import pytest

import momentum_numpy as M
import nemolite_boxes as NB
import open_bc_numpy as B
import oracle_lib as O
from nemolite_boxes import INS, MOM, OUTS, PRM

pytestmark = pytest.mark.gpu

CASES = NB.cases()
IDS = [NB.case_id(k, c) for k, c in enumerate(CASES)]
SSH_BC = 0.0625


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


def _setup(case, seed):
    """mask, host grid, inputs (MOM's ten arrays) and outputs (ssha distinct values, the others sentinels) of a case"""
    rng = np.random.default_rng(seed)
    tm = NB.mask(rng, case.ny, case.ld)
    G = NB.host_grid(rng, tm)
    shape = (case.ny, case.ld)
    H = NB._host_inputs(rng, shape)
    H["ssha_u"] = 0.1 * rng.normal(size=shape)
    H["ssha_v"] = 0.1 * rng.normal(size=shape)
    return tm, G, H, NB._host_outputs(rng, shape)


def _unchanged(dev, host):
    for k, a in host.items():
        got = dev[k].cpu().numpy()
        assert (M.same(got, a) if a.dtype == np.float64 else np.array_equal(got, a)), k


def _restated_step(G, tm, tbox, ubox, vbox, plan, H, Ho):
    """the step as DESIGN.md section 6.7 defines it, on the CPU: continuity -> bc_ssh -> next_sshu / next_sshv -> momentum
    -> Flather u / v"""
    W = {k: v.copy() for k, v in Ho.items()}
    ld = tm.shape[1]
    with np.errstate(all="ignore"):
        O.continuity_slabs(PRM[0], ld, tbox, H["sshn_t"], H["sshn_u"], H["sshn_v"], H["hu"], H["hv"], H["un"], H["vn"],
                           G.area_t, W["ssha"])
        if plan:
            B.bc_ssh(tbox, tm, SSH_BC, W["ssha"])
        M.next_sshu(ubox, tm, G.area_t, G.area_u, W["ssha"], W["ssha_u"])
        M.next_sshv(vbox, tm, G.area_t, G.area_v, W["ssha"], W["ssha_v"])
        hp = M.params(*PRM)
        M.momentum(hp, G, ubox, vbox, *[(H if k in INS else W)[k] for k in MOM], W["ua"], W["va"])
        if plan:
            B.flather_u(hp, ubox, tm, H["hu"], H["sshn_u"], H["sshn_t"], W["ua"])
            B.flather_v(hp, vbox, tm, H["hv"], H["sshn_v"], H["sshn_t"], W["va"])
    return W


# ---- momentum -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_momentum(D, case, kernel):
    """momentum_u on ubox, momentum_v on vbox, the fused entry on (ubox, vbox): every cell against momentum_numpy.
    kernel 0: the tile where the alignment allows it (the bounding box of U and V); 1: the one-cell form"""
    import torch
    L = D._cabi.lib()
    ld, ny, _, ubox, vbox, shift = case
    tm, Gh, H, _ = _setup(case, 11 * ld + ny)
    G, gdev, mg = NB.grid_on_device(torch, Gh)
    Dv = NB._dev(torch, H, shift)
    sent = {k: np.full((ny, ld), -7.0) for k in ("u", "v", "fu", "fv")}
    out = NB._dev(torch, sent, shift)
    prm = D.psy.momentum_params(*PRM)
    ins = [_p(Dv[k]) for k in MOM]
    try:
        _set_tuning(D, mom_kernel=kernel)
        D._cabi.check(L.dlesm_momentum_u_f64(C.byref(prm), C.byref(mg), ld, ny, *ubox, *ins[:9], _p(out["u"]), None))
        D._cabi.check(L.dlesm_momentum_v_f64(C.byref(prm), C.byref(mg), ld, ny, *vbox, *ins[:8], ins[9], _p(out["v"]), None))
        D._cabi.check(L.dlesm_momentum_f64(C.byref(prm), C.byref(mg), ld, ny, C.byref(D._cabi.Region(0, 0, *ubox)),
                                           C.byref(D._cabi.Region(0, 0, *vbox)), *ins, _p(out["fu"]), _p(out["fv"]), None))
        torch.cuda.synchronize()
    finally:
        _set_tuning(D, mom_kernel=0)
    hp = M.params(*PRM)
    want_u, want_v = np.full((ny, ld), -7.0), np.full((ny, ld), -7.0)
    M.momentum_u(hp, G, ubox, *[H[k] for k in MOM[:9]], want_u)
    M.momentum_v(hp, G, vbox, *[H[k] for k in MOM[:8]], H["ssha_v"], want_v)
    for k, want in (("u", want_u), ("fu", want_u), ("v", want_v), ("fv", want_v)):
        assert M.same(out[k].cpu().numpy(), want), k
    _unchanged(Dv, H)
    _unchanged(gdev, Gh)
    if not NB.empty(ubox) and (ubox[1] - ubox[0] + 1) * (ubox[3] - ubox[2] + 1) > 40:
        assert (want_u != -7.0).any()


# ---- next_sshu / next_sshv ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_next_ssh(D, case):
    import torch
    L = D._cabi.lib()
    ld, ny, _, ubox, vbox, shift = case
    tm, Gh, H, _ = _setup(case, 13 * ld + ny)
    G, gdev, _ = NB.grid_on_device(torch, Gh)
    Dv = NB._dev(torch, {"sshn_t": H["sshn_t"]}, shift)
    out = NB._dev(torch, {"u": np.full((ny, ld), -7.0), "v": np.full((ny, ld), -7.0)}, shift)
    D._cabi.check(L.dlesm_next_sshu_f64(ld, ny, *ubox, _p(gdev["tmask"]), _p(gdev["area_t"]), _p(gdev["area_u"]),
                                        _p(Dv["sshn_t"]), _p(out["u"]), None))
    D._cabi.check(L.dlesm_next_sshv_f64(ld, ny, *vbox, _p(gdev["tmask"]), _p(gdev["area_t"]), _p(gdev["area_v"]),
                                        _p(Dv["sshn_t"]), _p(out["v"]), None))
    torch.cuda.synchronize()
    for k, fn, area, box in (("u", M.next_sshu, G.area_u, ubox), ("v", M.next_sshv, G.area_v, vbox)):
        want = np.full((ny, ld), -7.0)
        fn(box, tm, G.area_t, area, H["sshn_t"], want)
        assert M.same(out[k].cpu().numpy(), want), k
    _unchanged(Dv, {"sshn_t": H["sshn_t"]})


# ---- the open boundary ----------------------------------------------------------------------------------------------
def _open_counts(tm, tbox, ubox, vbox):
    def faces(box, di, dj):
        if NB.empty(box):
            return 0
        S = B._view(box)
        a, b = S(tm), S(tm, di, dj)
        return int((((a < 0) & (b > 0)) | ((a > 0) & (b < 0))).sum())
    nt = 0 if NB.empty(tbox) else int((B._view(tbox)(tm) < 0).sum())
    return nt, faces(ubox, 1, 0), faces(vbox, 0, 1)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_open_boundary(D, case):
    """a plan on (tbox, ubox, vbox), then bc_open: every cell against open_bc_numpy; the plan's counts against the open
    cells and faces the restatement finds"""
    import torch
    L = D._cabi.lib()
    ld, ny, tbox, ubox, vbox, shift = case
    rng = np.random.default_rng(17 * ld + ny)
    tm = NB.mask(rng, ny, ld)
    shape = (ny, ld)
    H = {"hu": 10.0 + rng.random(shape), "hv": 10.0 + rng.random(shape)}
    for k in ("sshn_u", "sshn_v", "sshn_t"):
        H[k] = 0.1 * rng.normal(size=shape)
    Ho = {"ssha": 1000.0 + rng.random(shape), "ua": NB._vel(rng, shape), "va": NB._vel(rng, shape)}
    Dv, Do = NB._dev(torch, H, shift), NB._dev(torch, Ho, shift)
    prm = D.psy.momentum_params(*PRM)
    plan = NB._plan(D, tm, tbox, ubox, vbox)
    try:
        n = [C.c_int(), C.c_int(), C.c_int()]
        D._cabi.check(L.dlesm_obc_counts(plan, *[C.byref(x) for x in n]))
        assert tuple(x.value for x in n) == _open_counts(tm, tbox, ubox, vbox)
        D._cabi.check(L.dlesm_bc_open_f64(plan, C.byref(prm), SSH_BC, *[_p(Dv[k]) for k in ("hu", "sshn_u", "hv", "sshn_v",
                                                                                            "sshn_t")],
                                          _p(Do["ssha"]), _p(Do["ua"]), _p(Do["va"]), None))
        torch.cuda.synchronize()
    finally:
        L.dlesm_obc_destroy(plan)
    want = {k: v.copy() for k, v in Ho.items()}
    B.bc_open(M.params(*PRM), tbox, ubox, vbox, tm, SSH_BC, H["hu"], H["sshn_u"], H["hv"], H["sshn_v"], H["sshn_t"],
              want["ssha"], want["ua"], want["va"])
    for k in Ho:
        assert M.same(Do[k].cpu().numpy(), want[k]), k
    _unchanged(Dv, H)


# ---- the one-call step ----------------------------------------------------------------------------------------------
def _step(D, case, tbox, ubox, vbox, with_plan, kernel, seed):
    """the one call on a case's arrays against the restated step; returns (tm, host outputs before, device outputs after)"""
    import torch
    ld, ny, shift = case.ld, case.ny, case.shift
    tm, Gh, H, Ho = _setup(case, seed)
    H = {k: H[k] for k in INS}
    G, gdev, mg = NB.grid_on_device(torch, Gh)
    I, O_ = NB._dev(torch, H, shift), NB._dev(torch, Ho, shift)
    prm = D.psy.momentum_params(*PRM)
    plan = NB._plan(D, tm, tbox, ubox, vbox) if with_plan else None
    try:
        _set_tuning(D, nemo_step_kernel=kernel)
        rc = D._cabi.lib().dlesm_nemolite_step_f64(C.byref(prm), C.byref(mg), _p(gdev["area_t"]), ld, ny,
                                                   C.byref(D._cabi.Region(0, 0, *tbox)),
                                                   C.byref(D._cabi.Region(0, 0, *ubox)),
                                                   C.byref(D._cabi.Region(0, 0, *vbox)), plan, SSH_BC,
                                                   *[_p(I[k]) for k in INS], *[_p(O_[k]) for k in OUTS], None)
        assert rc == 0, D._cabi.lib().dlesm_last_error()
        torch.cuda.synchronize()
    finally:
        _set_tuning(D, nemo_step_kernel=0)
        if plan is not None:
            D._cabi.lib().dlesm_obc_destroy(plan)
    got = {k: O_[k].cpu().numpy() for k in OUTS}
    want = _restated_step(G, tm, tbox, ubox, vbox, with_plan, H, Ho)
    for k in OUTS:
        assert M.same(got[k], want[k]), k
    _unchanged(I, H)
    _unchanged(gdev, Gh)
    return tm, Ho, got


@pytest.mark.parametrize("with_plan", [False, True])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_step_tile(D, case, with_plan):
    """tbox = ubox = vbox = the case's tbox, nemo_step_kernel 0: the wave tile on even ld and aligned bases; the ring's
    ssha (east column, north row) is read and never written"""
    box = case.tbox
    k = CASES.index(case)
    if k < NB.N_FIXED:
        assert NB.tile_case(case)                       # the fixed edge placements reach the tile
    tm, Ho, got = _step(D, case, box, box, box, with_plan, 0, 19 * case.ld + case.ny + k)
    if not NB.empty(box):
        x0, x1, y0, y1 = box
        assert M.same(got["ssha"][y1, x0 - 1:x1 + 1], Ho["ssha"][y1, x0 - 1:x1 + 1])    # the north ring row
        assert M.same(got["ssha"][y0 - 1:y1 + 1, x1], Ho["ssha"][y0 - 1:y1 + 1, x1])    # the east ring column


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_step_definition(D, case, kernel):
    """the case's own three boxes with an open-boundary plan: independent boxes take the definition path; kernel 1
    forces it on equal boxes too"""
    k = CASES.index(case)
    if kernel == 0 and case.tbox == case.ubox == case.vbox:
        # equal boxes: the tile again, on three independent random boxes of the same arrays instead
        rng = np.random.default_rng(k)
        boxes = [NB._rand_box(rng, case.ld, case.ny) for _ in range(3)]
    else:
        boxes = [case.tbox, case.ubox, case.vbox]
    _step(D, case, *boxes, True, kernel, 23 * case.ld + case.ny + k)


# ---- IEEE special values --------------------------------------------------------------------------------------------
SPECIAL_SHAPES = [(256, 12, (2, 255, 2, 11)), (130, 9, (5, 100, 3, 8)), (1002, 6, (2, 1001, 2, 5)), (129, 10, (2, 128, 2, 9))]


def _written(after, before):
    """the cells a call wrote (a written NaN over a NaN sentinel cannot happen: sentinels are finite)"""
    return ~((after.view(np.uint64) == before.view(np.uint64)))


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("ld,ny,box", SPECIAL_SHAPES)
def test_special_values_momentum(D, ld, ny, box, kernel):
    """the fused momentum entry on inputs with subnormals, signed zeros, infinities, NaN of both signs, 1e300-scale
    products and exactly zero denominators: every cell against momentum_numpy, and the outputs hold infinities, NaN and
    subnormals in written cells"""
    import torch
    L = D._cabi.lib()
    tm, Gh, H, _ = NB.special_inputs(ld * 3 + ny, ld, ny)
    G, gdev, mg = NB.grid_on_device(torch, Gh)
    Dv = NB._dev(torch, H, 0)
    ua, va = (torch.full((ny, ld), -7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    prm = D.psy.momentum_params(*PRM)
    try:
        _set_tuning(D, mom_kernel=kernel)
        r = D._cabi.Region(0, 0, *box)
        D._cabi.check(L.dlesm_momentum_f64(C.byref(prm), C.byref(mg), ld, ny, C.byref(r), C.byref(r),
                                           *[_p(Dv[k]) for k in MOM], _p(ua), _p(va), None))
        torch.cuda.synchronize()
    finally:
        _set_tuning(D, mom_kernel=0)
    want_u, want_v = np.full((ny, ld), -7.0), np.full((ny, ld), -7.0)
    with np.errstate(all="ignore"):
        M.momentum(M.params(*PRM), G, box, box, *[H[k] for k in MOM], want_u, want_v)
    gu, gv = ua.cpu().numpy(), va.cpu().numpy()
    assert M.same(gu, want_u) and M.same(gv, want_v)
    _unchanged(Dv, H)
    w = np.concatenate([gu[_written(gu, np.full_like(gu, -7.0))], gv[_written(gv, np.full_like(gv, -7.0))]])
    assert np.isinf(w).any() and np.isnan(w).any() and NB.is_subnormal(w).any()


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("ld,ny,box", SPECIAL_SHAPES)
def test_special_values_step(D, ld, ny, box, kernel):
    """the one-call step on the same inputs (the step's own zero denominators in the calm patch): every cell of every
    output against the restated step"""
    import torch
    tm, Gh, H, Ho = NB.special_inputs(ld * 5 + ny, ld, ny)
    H = {k: H[k] for k in INS}
    G, gdev, mg = NB.grid_on_device(torch, Gh)
    I, O_ = NB._dev(torch, H, 0), NB._dev(torch, Ho, 0)
    prm = D.psy.momentum_params(*PRM)
    try:
        _set_tuning(D, nemo_step_kernel=kernel)
        rc = D._cabi.lib().dlesm_nemolite_step_f64(C.byref(prm), C.byref(mg), _p(gdev["area_t"]), ld, ny,
                                                   *[C.byref(D._cabi.Region(0, 0, *box))] * 3, None, 0.0,
                                                   *[_p(I[k]) for k in INS], *[_p(O_[k]) for k in OUTS], None)
        assert rc == 0, D._cabi.lib().dlesm_last_error()
        torch.cuda.synchronize()
    finally:
        _set_tuning(D, nemo_step_kernel=0)
    got = {k: O_[k].cpu().numpy() for k in OUTS}
    want = _restated_step(G, tm, box, box, box, False, H, Ho)
    for k in OUTS:
        assert M.same(got[k], want[k]), k
    _unchanged(I, H)
    w = np.concatenate([got[k][_written(got[k], Ho[k])] for k in OUTS])
    assert np.isinf(w).any() and np.isnan(w).any() and NB.is_subnormal(w).any()
    calm = (slice(ny // 3, ny // 3 + 3), slice(ld // 3, ld // 3 + 6))
    assert (got["ssha_u"][calm] == 0.0).any() and np.isnan(got["ua"][calm]).any()      # hu + ssha_u = 0 reached
