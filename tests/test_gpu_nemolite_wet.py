"""GPU tests (-m gpu) of the NEMOLite2D-class time step that skips land: the wet plan
(dlesm_wet_plan_*), dlesm_nemolite_step_wet_f64 and dlesm_nemolite_step_wet_dm.  The yardstick is always the existing entry
(dlesm_nemolite_step_f64, dlesm_nemolite_step_dm) run on copies of the same inputs in the same test, and the contract is

  * ssha_u, ssha_v, ua, va: the yardstick's bits in EVERY cell -- box, ring and padding;
  * ssha: the yardstick's bits in every cell with T != 0 and in every cell outside tbox; a T == 0 cell of tbox holds either
    the yardstick's value or its content from before the call;
  * inputs untouched.

Arrays are 520 x 40 unless stated: four to five wave tiles per row, the smallest size at which a tile can be wholly land with
active neighbours on every side.  Outputs start as nemolite_boxes._host_outputs gives them (distinct ssha, -7.0 elsewhere).
Both forms of the kernel run: the flag map (the default) and the compacted list (HOOK key nemo_wet_form = 1)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import momentum_numpy as M
import nemolite_boxes as NB
import open_bc_numpy as B
import oracle_lib as O
from nemolite_boxes import INS, METRICS, MOM, OUTS, PRM, _dev, _host_inputs, _host_outputs, _plan, _raw_grid

pytestmark = pytest.mark.gpu
LD, NY = 520, 40
BOX = (2, LD - 1, 2, NY - 1)
SSH_BC = 0.0625


@pytest.fixture(scope="module")
def D():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    import dl_esm_inf_amd as d
    torch.cuda.set_device(0)
    d.parallel_init(0, 1, use_rccl=True)
    return d


def _p(t):
    return C.c_void_p(t.data_ptr())


def _R(D, box):
    return C.byref(D._cabi.Region(0, 0, *box))


# ---- masks ----------------------------------------------------------------------------------------------------------
def all_wet(ld=LD, ny=NY):
    return np.ones((ny, ld), dtype=np.int32)


def zeros(ld=LD, ny=NY):
    return np.zeros((ny, ld), dtype=np.int32)


def continent(seed=7, ld=LD, ny=NY):
    """land in columns 61..460, rows 6..30 (400 columns: whole tiles under any anchoring of a <= 126-column tile), random
    -1/0/1 elsewhere, repaired for the open-boundary plan"""
    rng = np.random.default_rng(seed)
    tm = rng.choice(np.array([-1, 0, 1, 1, 1], dtype=np.int32), size=(ny, ld))
    tm[6:31, 61:461] = 0
    return B.repair(tm)


LONE_NY = 100
LONE_COLS = list(range(120, 136)) + list(range(246, 261))


def lone_cells():
    """520 x 100, all land but single wet cells, one per row in rows 3, 6, 9, ..., each at another column of 120..135 and
    246..260: wherever the tile seams fall, some wet cell is the first column of a tile beside an all-land tile, and some
    sits directly above an all-land tile -- the ssha_u / ssha_v stores on the land cells west and south of it are the only
    stores of those tiles"""
    tm = zeros(LD, LONE_NY)
    for k, col in enumerate(LONE_COLS):
        tm[3 + 3 * k, col] = 1
    assert 3 + 3 * (len(LONE_COLS) - 1) < LONE_NY - 1
    return tm


# ---- the plan, the calls, the contract ----------------------------------------------------------------------------------
def _wet(D, tm, box, ld=None, ny=None):
    tm = np.ascontiguousarray(tm, dtype=np.int32)
    h = C.c_void_p()
    D._cabi.check(D._cabi.lib().dlesm_wet_plan_create(tm.ctypes.data, ld or tm.shape[1], ny or tm.shape[0], _R(D, box),
                                                      C.byref(h)))
    return h


def _counts(D, h):
    t, a = C.c_longlong(), C.c_longlong()
    D._cabi.check(D._cabi.lib().dlesm_wet_plan_counts(h, C.byref(t), C.byref(a)))
    return t.value, a.value


def _step(D, wet, prm, mg, gdev, ld, ny, boxes, obc, ssh_bc, I, O_, plain=False):
    args = (C.byref(prm), C.byref(mg), _p(gdev["area_t"]), ld, ny, *[_R(D, b) for b in boxes], obc, ssh_bc,
            *[_p(I[k]) for k in INS], *[_p(O_[k]) for k in OUTS], None)
    L = D._cabi.lib()
    return L.dlesm_nemolite_step_f64(*args) if plain else L.dlesm_nemolite_step_wet_f64(wet, *args)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def contract(tm, tbox, got, ref, before):
    """the contract of section 6.9 on host arrays; returns the number of T == 0 cells of tbox that kept their content"""
    for k in OUTS[1:]:
        assert M.same(got[k], ref[k]), (k, np.argwhere(_bits(got[k]) != _bits(ref[k]))[:5])
    land = np.zeros(tm.shape, dtype=bool)
    x0, x1, y0, y1 = tbox
    if x1 >= x0 and y1 >= y0:
        land[y0 - 1:y1, x0 - 1:x1] = tm[y0 - 1:y1, x0 - 1:x1] == 0
    g, r, b = got["ssha"], ref["ssha"], before["ssha"]
    assert M.same(g[~land], r[~land]), np.argwhere(~land & (_bits(g) != _bits(r)))[:5]
    as_ref = (_bits(g) == _bits(r)) | (np.isnan(g) & np.isnan(r))
    kept = _bits(g) == _bits(b)
    assert bool(np.all((as_ref | kept)[land])), np.argwhere(land & ~as_ref & ~kept)[:5]
    return int(np.count_nonzero(land & kept & ~as_ref))


def _host(T):
    return {k: v.cpu().numpy() for k, v in T.items()}


def _forms(D, fn):
    """run fn under both forms of the kernel"""
    L = D._cabi.lib()
    out = []
    for form in (0, 1):
        L.dlesm_set_tuning(b"nemo_wet_form", form)
        try:
            out.append(fn())
        finally:
            L.dlesm_set_tuning(b"nemo_wet_form", 0)
    return out


def _one_step(D, tm, boxes, with_obc, seed, shift=0, kernel=0):
    """one step with the plan against the existing entry; returns (tiles, active, land cells that kept their content) per form"""
    import torch
    L = D._cabi.lib()
    ny, ld = tm.shape
    rng = np.random.default_rng(seed)
    G, gdev, mg = _raw_grid(torch, rng, tm)
    Hi, Ho = _host_inputs(rng, (ny, ld)), _host_outputs(rng, (ny, ld))
    I = _dev(torch, Hi, shift)
    prm = D.psy.momentum_params(*PRM)
    obc = _plan(D, tm, *boxes) if with_obc else None
    wet = _wet(D, tm, boxes[0])
    try:
        L.dlesm_set_tuning(b"nemo_step_kernel", kernel)
        Oref = _dev(torch, Ho, shift)
        assert _step(D, None, prm, mg, gdev, ld, ny, boxes, obc, SSH_BC, I, Oref, plain=True) == 0, L.dlesm_last_error()
        torch.cuda.synchronize()
        ref = _host(Oref)

        def run():
            Owet = _dev(torch, Ho, shift)
            assert _step(D, wet, prm, mg, gdev, ld, ny, boxes, obc, SSH_BC, I, Owet) == 0, L.dlesm_last_error()
            torch.cuda.synchronize()
            kept = contract(tm, boxes[0], _host(Owet), ref, Ho)
            for k in INS:
                assert M.same(I[k].cpu().numpy(), Hi[k]), k
            return (*_counts(D, wet), kept)
        return _forms(D, run)
    finally:
        L.dlesm_set_tuning(b"nemo_step_kernel", 0)
        L.dlesm_wet_plan_destroy(wet)
        if obc is not None:
            L.dlesm_obc_destroy(obc)


# ---- 1. counts ------------------------------------------------------------------------------------------------------------
def test_counts(D):
    L = D._cabi.lib()
    got = {}
    for name, tm in (("wet", all_wet()), ("zeros", zeros()), ("continent", continent()), ("lone", lone_cells())):
        h = _wet(D, tm, (2, tm.shape[1] - 1, 2, tm.shape[0] - 1))
        got[name] = _counts(D, h)
        L.dlesm_wet_plan_destroy(h)
    tiles, active = got["wet"]
    assert active == tiles > 0
    assert got["zeros"] == (tiles, 0)
    assert got["continent"][0] == tiles and 0 < got["continent"][1] < tiles
    # a lone wet cell makes active its own tile, the tile below it and, where it is the first column of a tile, the tile west
    t, a = got["lone"]
    assert 2 * len(LONE_COLS) <= a <= 4 * len(LONE_COLS) < t
    h = _wet(D, all_wet(), (5, 4, 2, 2))                     # an empty box: a plan of no tiles
    assert _counts(D, h) == (0, 0)
    L.dlesm_wet_plan_destroy(h)
    assert L.dlesm_wet_plan_destroy(None) == 0


# ---- 2. one step obeys the contract; 3. it really skips ----------------------------------------------------------------------
@pytest.mark.parametrize("with_obc", [False, True])
@pytest.mark.parametrize("name", ["wet", "zeros", "continent", "lone"])
def test_one_step_obeys_the_contract(D, name, with_obc):
    tm = {"wet": all_wet, "zeros": zeros, "continent": continent, "lone": lone_cells}[name]()
    box = (2, tm.shape[1] - 1, 2, tm.shape[0] - 1)
    for tiles, active, kept in _one_step(D, tm, (box,) * 3, with_obc, 100 + len(name)):
        if name == "wet":
            assert active == tiles and kept == 0
        elif name == "zeros":
            assert active == 0 and kept == (tm.shape[1] - 2) * (tm.shape[0] - 2)    # every box cell kept its ssha
        else:
            assert 0 < active < tiles and kept > 0                               # it really skips


def test_all_land_writes_nothing(D):
    """the mask of zeros: all five outputs are untouched in every cell"""
    import torch
    tm = zeros()
    rng = np.random.default_rng(3)
    G, gdev, mg = _raw_grid(torch, rng, tm)
    Hi, Ho = _host_inputs(rng, (NY, LD)), _host_outputs(rng, (NY, LD))
    I = _dev(torch, Hi, 0)
    wet = _wet(D, tm, BOX)
    try:
        def run():
            O_ = _dev(torch, Ho, 0)
            assert _step(D, wet, D.psy.momentum_params(*PRM), mg, gdev, LD, NY, (BOX,) * 3, None, 0.0, I, O_) == 0
            torch.cuda.synchronize()
            for k in OUTS:
                assert M.same(O_[k].cpu().numpy(), Ho[k]), k
        _forms(D, run)
    finally:
        D._cabi.lib().dlesm_wet_plan_destroy(wet)


SUBBOXES = [c for c in NB.cases() if NB.tile_case(c) and c.tbox == c.ubox == c.vbox and not NB.empty(c.tbox)
            and c.tbox[0] > 16 and c.tbox[3] - c.tbox[2] >= 2 and c.tbox[1] - c.tbox[0] >= 60][:3]


@pytest.mark.parametrize("with_obc", [False, True])
@pytest.mark.parametrize("case", SUBBOXES, ids=[f"ld{c.ld}x{c.ny}-x{c.tbox[0]}" for c in SUBBOXES])
def test_boxes_away_from_the_origin(D, case, with_obc):
    """equal-box cases of nemolite_boxes.cases whose box starts away from the origin (the tiles anchor on the box): a random
    mask with a band of land across the middle rows of the box"""
    assert len(SUBBOXES) == 3
    rng = np.random.default_rng(case.ld + case.ny)
    tm = rng.choice(np.array([-1, 0, 1, 1, 1], dtype=np.int32), size=(case.ny, case.ld))
    x0, x1, y0, y1 = case.tbox
    tm[y0:y1 - 1, :] = 0                                   # (0-based rows y0 .. y1-2: all but the first and last row of the box)
    tm = B.repair(tm)
    _one_step(D, tm, (case.tbox,) * 3, with_obc, case.ld)


# ---- 4. the definition path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld,boxes,shift,kernel", [
    (301, None, 0, 0),                                                             # an odd leading dimension
    (LD, None, 1, 0),                                                              # bases 8 bytes off a 16-byte boundary
    (LD, ((37, 450, 5, 36), (40, 518, 2, 39), (2, 519, 9, 30)), 0, 0),            # three unequal boxes
    (LD, None, 0, 1),                                                              # the HOOK key nemo_step_kernel = 1
])
def test_definition_path(D, ld, boxes, shift, kernel):
    """the plan may be ignored; the contract holds"""
    tm = continent(9, ld=ld) if ld == LD else B.repair(_land_block(301))
    box = (2, ld - 1, 2, NY - 1)
    _one_step(D, tm, boxes or (box,) * 3, True, 40 + ld + shift + kernel, shift=shift, kernel=kernel)


def _land_block(ld):
    rng = np.random.default_rng(ld)
    tm = rng.choice(np.array([-1, 0, 1, 1, 1], dtype=np.int32), size=(NY, ld))
    tm[6:31, 20:ld - 20] = 0
    return tm


# ---- 5. a time loop -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1])
def test_time_loop(D, form):
    """eight tidal steps with pointer rotation on the continent mask, with the plan and without, from the same state: after
    every step the four face arrays are identical everywhere and ssha where T != 0; after the last step the same cells equal
    the CPU restatements run in DESIGN.md section 6.6's order"""
    import torch
    L = D._cabi.lib()
    tm = continent(21)
    rng = np.random.default_rng(21)
    G, gdev, mg = _raw_grid(torch, rng, tm)
    H = {**_host_inputs(rng, (NY, LD)), **_host_outputs(rng, (NY, LD))}
    for k in ("un", "vn"):
        H[k] *= 0.1
    A, R = _dev(torch, H, 0), _dev(torch, H, 0)
    prm, hp = D.psy.momentum_params(*PRM), M.params(*PRM)
    obc, wet = _plan(D, tm, BOX, BOX, BOX), _wet(D, tm, BOX)
    wetc = tm != 0
    omega = 2.0 * math.pi / 43200.0
    rot = (("un", "ua"), ("vn", "va"), ("sshn_t", "ssha"), ("sshn_u", "ssha_u"), ("sshn_v", "ssha_v"))
    L.dlesm_set_tuning(b"nemo_wet_form", form)
    try:
        for step in range(8):
            ssh_bc = D.psy.tide_ssh(0.1, omega, (step + 1) * PRM[0])
            assert _step(D, None, prm, mg, gdev, LD, NY, (BOX,) * 3, obc, ssh_bc, R, R, plain=True) == 0
            assert _step(D, wet, prm, mg, gdev, LD, NY, (BOX,) * 3, obc, ssh_bc, A, A) == 0, L.dlesm_last_error()
            torch.cuda.synchronize()
            a, r = _host(A), _host(R)
            for k in OUTS[1:]:
                assert M.same(a[k], r[k]), (step, k)
            assert M.same(a["ssha"][wetc], r["ssha"][wetc]), step
            # the CPU restatements, section 6.6's order
            O.continuity_slabs(PRM[0], LD, BOX, H["sshn_t"], H["sshn_u"], H["sshn_v"], H["hu"], H["hv"], H["un"], H["vn"],
                               G.area_t, H["ssha"])
            B.bc_ssh(BOX, tm, B.tide(0.1, omega, (step + 1) * PRM[0]), H["ssha"])
            M.next_sshu(BOX, tm, G.area_t, G.area_u, H["ssha"], H["ssha_u"])
            M.next_sshv(BOX, tm, G.area_t, G.area_v, H["ssha"], H["ssha_v"])
            M.momentum(hp, G, BOX, BOX, *[H[k] for k in MOM], H["ua"], H["va"])
            B.flather_u(hp, BOX, tm, H["hu"], H["sshn_u"], H["sshn_t"], H["ua"])
            B.flather_v(hp, BOX, tm, H["hv"], H["sshn_v"], H["sshn_t"], H["va"])
            for X in (A, R, H):
                for p, q in rot:
                    X[p], X[q] = X[q], X[p]
        a = _host(A)
        for k in ("sshn_u", "sshn_v", "un", "vn"):                               # (rotated: the last step's outputs)
            assert M.same(a[k], H[k]), k
        assert M.same(a["sshn_t"][wetc], H["sshn_t"][wetc])
        assert not M.same(a["sshn_t"], _host(R)["sshn_t"])                       # land ssha did go stale
        assert np.isfinite(a["un"]).all() and (a["un"] != -7.0).any()
    finally:
        L.dlesm_set_tuning(b"nemo_wet_form", 0)
        L.dlesm_wet_plan_destroy(wet)
        L.dlesm_obc_destroy(obc)


# ---- 6. wet == NULL -----------------------------------------------------------------------------------------------------
def test_null_plan_is_the_existing_entry(D):
    """every cell of every output, land ssha included"""
    import torch
    tm = continent(5)
    rng = np.random.default_rng(5)
    G, gdev, mg = _raw_grid(torch, rng, tm)
    Hi, Ho = _host_inputs(rng, (NY, LD)), _host_outputs(rng, (NY, LD))
    I, O0, O1 = _dev(torch, Hi, 0), _dev(torch, Ho, 0), _dev(torch, Ho, 0)
    prm = D.psy.momentum_params(*PRM)
    obc = _plan(D, tm, BOX, BOX, BOX)
    try:
        assert _step(D, None, prm, mg, gdev, LD, NY, (BOX,) * 3, obc, SSH_BC, I, O0, plain=True) == 0
        assert _step(D, None, prm, mg, gdev, LD, NY, (BOX,) * 3, obc, SSH_BC, I, O1) == 0
        torch.cuda.synchronize()
        for k in OUTS:
            assert M.same(O1[k].cpu().numpy(), O0[k].cpu().numpy()), k
        assert not M.same(O1["ssha"].cpu().numpy(), Ho["ssha"])
    finally:
        D._cabi.lib().dlesm_obc_destroy(obc)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals(D):
    """a plan for another ld, for another ny, for another box: DLESM_EINVAL with all five outputs untouched; the plan's own
    refusals"""
    import torch
    L = D._cabi.lib()
    tm = continent(6)
    rng = np.random.default_rng(6)
    G, gdev, mg = _raw_grid(torch, rng, tm)
    Hi, Ho = _host_inputs(rng, (NY, LD)), _host_outputs(rng, (NY, LD))
    I, O_ = _dev(torch, Hi, 0), _dev(torch, Ho, 0)
    prm = D.psy.momentum_params(*PRM)
    plans = [(_wet(D, continent(6, ld=LD + 2), BOX), b"wet plan was made for 522x40"),
             (_wet(D, continent(6, ny=NY + 1), BOX), b"wet plan was made for 520x41"),
             (_wet(D, tm, (2, LD - 1, 3, NY - 1)), b"wet plan was made for the box")]
    try:
        for form in (0, 1):
            L.dlesm_set_tuning(b"nemo_wet_form", form)
            for h, msg in plans:
                rc = _step(D, h, prm, mg, gdev, LD, NY, (BOX,) * 3, None, 0.0, I, O_)
                assert rc == D._cabi.EINVAL and msg in L.dlesm_last_error(), (rc, L.dlesm_last_error())
        torch.cuda.synchronize()
        for k in OUTS:
            assert M.same(O_[k].cpu().numpy(), Ho[k]), k
    finally:
        L.dlesm_set_tuning(b"nemo_wet_form", 0)
        for h, _ in plans:
            L.dlesm_wet_plan_destroy(h)
    h = C.c_void_p()
    t32 = np.ascontiguousarray(tm)
    assert L.dlesm_wet_plan_create(None, LD, NY, _R(D, BOX), C.byref(h)) == D._cabi.EINVAL
    assert L.dlesm_wet_plan_create(t32.ctypes.data, LD, NY, None, C.byref(h)) == D._cabi.EINVAL
    assert L.dlesm_wet_plan_create(t32.ctypes.data, LD, NY, _R(D, BOX), None) == D._cabi.EINVAL
    assert L.dlesm_wet_plan_create(t32.ctypes.data, LD, NY, _R(D, (1, LD, 2, NY - 1)), C.byref(h)) == D._cabi.EINVAL   # no ring
    assert not h.value
    n = C.c_longlong()
    assert L.dlesm_wet_plan_counts(None, C.byref(n), C.byref(n)) == D._cabi.EINVAL


# ---- 8. the distributed entry -------------------------------------------------------------------------------------------
def _dm_case(D, DM, peer, tables=True):
    """test_gpu_nemolite_step_dm's loop-back case on the continent mask: no open cell but an open west column, land in the last
    internal column, and the ring of the mask the periodic image of the interior (a halo cell is masked as its source cell)"""
    import torch
    S = DM.Case(D, LD, NY, 31 + peer, peer=peer, tables=tables)
    rng = np.random.default_rng(8)
    tm = rng.choice(np.array([0, 1, 1, 1], dtype=np.int32), size=(NY, LD))
    tm[6:31, 61:461] = 0
    tm[:, 1] = -1
    tm[:, LD - 2] = 0
    if tables:
        oc = O.Comms()
        C.memmove(C.byref(oc), C.byref(S.t), C.sizeof(oc))
        f = tm.astype(np.float64)
        assert O.exchange_all([f], [LD], [oc]) == 0
        tm = f.astype(np.int32)
    tm = np.ascontiguousarray(tm)
    assert B.refusal(tm, S.box, S.box) is None
    S.tm = tm
    S.gdev["tmask"].copy_(torch.from_numpy(tm))
    torch.cuda.synchronize()
    return S


def _wet_dm(S, wet, I, O_, obc, ssh_bc, prm):
    return S.L.dlesm_nemolite_step_wet_dm(S.plan, wet, C.byref(prm), C.byref(S.mg), _p(S.gdev["area_t"]), S.ld, S.ny,
                                          *[_R(S.D, S.box)] * 3, obc, ssh_bc, *[_p(I[k]) for k in INS],
                                          *[_p(O_[k]) for k in OUTS], None)


@pytest.mark.parametrize("peer", [0, 3])
@pytest.mark.parametrize("with_obc", [False, True])
def test_distributed_entry_in_loopback(D, peer, with_obc):
    """over the RCCL group and over the mailboxes (the exchange in two turns): the face arrays equal dlesm_nemolite_step_dm's
    in every cell, halos included; ssha obeys the contract on the box and its halos are the images of the interior -- stale
    land ssha travels in the exchange"""
    import torch
    import test_gpu_nemolite_step_dm as DM
    S = _dm_case(D, DM, peer)
    wet = _wet(D, S.tm, S.box)
    try:
        prm = D.psy.momentum_params(*PRM)
        obc = S.make_obc() if with_obc else None
        tiles, active = _counts(D, wet)
        assert 0 < active < tiles
        Oref = S.outputs()
        assert DM.one_call(S, S.I, Oref, obc, SSH_BC, prm) == 0, S.L.dlesm_last_error()
        torch.cuda.synchronize()
        ref = _host(Oref)
        # a null wet plan: dlesm_nemolite_step_dm in every cell
        O0 = S.outputs()
        assert _wet_dm(S, None, S.I, O0, obc, SSH_BC, prm) == 0, S.L.dlesm_last_error()
        torch.cuda.synchronize()
        for k in OUTS:
            assert M.same(O0[k].cpu().numpy(), ref[k]), k
        oc = O.Comms()
        C.memmove(C.byref(oc), C.byref(S.t), C.sizeof(oc))
        inner = np.zeros((NY, LD), dtype=bool)
        inner[1:-1, 1:-1] = True

        def run():
            O1 = S.outputs()
            assert _wet_dm(S, wet, S.I, O1, obc, SSH_BC, prm) == 0, S.L.dlesm_last_error()
            torch.cuda.synchronize()
            got = _host(O1)
            for k in OUTS[1:]:
                assert M.same(got[k], ref[k]), k
            g = got["ssha"]
            img = g.copy()
            assert O.exchange_all([img], [LD], [oc]) == 0
            assert M.same(img, g)                                          # the halos: images of the interior
            wetc = S.tm != 0
            assert M.same(g[wetc], ref["ssha"][wetc])                      # (halo cells included: masked as their sources)
            box_only = {k: np.where(inner, got[k], ref[k]) for k in OUTS}
            assert contract(S.tm, S.box, box_only, ref, S.Ho) > 0
            for k in INS:
                assert M.same(S.I[k].cpu().numpy(), S.Hi[k]), k
        _forms(D, run)
        # refused before anything is launched or exchanged
        other = _wet(D, S.tm, (2, LD - 1, 3, NY - 1))
        O2 = S.outputs()
        assert _wet_dm(S, other, S.I, O2, obc, SSH_BC, prm) == D._cabi.EINVAL
        S.L.dlesm_wet_plan_destroy(other)
        torch.cuda.synchronize()
        for k in OUTS:
            assert M.same(O2[k].cpu().numpy(), S.Ho[k]), k
    finally:
        S.L.dlesm_wet_plan_destroy(wet)
        S.close()


def test_distributed_entry_without_messages_is_the_single_domain_entry(D):
    import torch
    import test_gpu_nemolite_step_dm as DM
    S = _dm_case(D, DM, 0, tables=False)
    wet = _wet(D, S.tm, S.box)
    try:
        prm = D.psy.momentum_params(*PRM)
        obc = S.make_obc()
        Os, O1 = S.outputs(), S.outputs()
        assert _step(D, wet, prm, S.mg, S.gdev, LD, NY, (S.box,) * 3, obc, SSH_BC, S.I, Os) == 0
        assert _wet_dm(S, wet, S.I, O1, obc, SSH_BC, prm) == 0, S.L.dlesm_last_error()
        torch.cuda.synchronize()
        for k in OUTS:
            assert M.same(O1[k].cpu().numpy(), Os[k].cpu().numpy()), k
        assert not M.same(O1["ua"].cpu().numpy(), S.Ho["ua"])
    finally:
        S.L.dlesm_wet_plan_destroy(wet)
        S.close()


# ---- 9. the Python wrappers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dm", [False, True])
def test_python_wrappers(D, dm):
    """skip_land=True against skip_land=False on a grid_init grid: a channel with open west and east columns, land rows north
    and south, and a land block 420 columns wide"""
    import torch
    nx, ny = 600, 40
    user = np.ones((ny + 2, nx + 2), dtype=np.int32)
    user[:, 0] = user[:, -1] = 0
    user[:, 1] = user[:, nx] = -1
    user[:3, :] = 0
    user[-3:, :] = 0
    user[8:30, 90:510] = 0
    os.environ["DL_ESM_ALIGNMENT"] = "64"
    try:
        g = D.grid_type(D.GO_ARAKAWA_C, (1, 1, 2), D.GO_OFFSET_NE)
        g.decompose(nx, ny)
        D.grid_init(g, 1000.0, 1000.0, tmask=user)
    finally:
        os.environ.pop("DL_ESM_ALIGNMENT", None)
    D.psy.coriolis(g)
    plan = D.psy.wet_plan(g)
    assert plan is D.psy.wet_plan(g) and 0 < plan.active < plan.tiles and "active" in repr(plan)
    rng = np.random.default_rng(17)
    shape = (g.ny, g.nx)
    H = {**_host_inputs(rng, shape), **_host_outputs(rng, shape)}
    T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
    pts = {"ssha": T, "sshn_t": T, "ht": T, "sshn_u": U, "ssha_u": U, "un": U, "ua": U, "hu": U,
           "sshn_v": V, "ssha_v": V, "vn": V, "va": V, "hv": V}
    F, F2 = {}, {}
    for k, a in H.items():
        F[k], F2[k] = D.r2d_field(g, pts[k]), D.r2d_field(g, pts[k])
        F[k].data.copy_(torch.from_numpy(a))
        F2[k].data.copy_(torch.from_numpy(a))
    prm = D.psy.momentum_params(*PRM)
    call = D.psy.invoke_nemolite_step_dm if dm else D.psy.invoke_nemolite_step
    call(prm, *[F[k] for k in OUTS], *[F[k] for k in INS], ssh_bc=0.03125)
    call(prm, *[F2[k] for k in OUTS], *[F2[k] for k in INS], ssh_bc=0.03125, skip_land=True)
    torch.cuda.synchronize()
    got, ref = {k: F2[k].get_data() for k in OUTS}, {k: F[k].get_data() for k in OUTS}
    assert contract(g.tmask, F["ssha"].internal.box(), got, ref, H) > 0
    for k in INS:
        assert M.same(F2[k].get_data(), H[k]), k
    assert (ref["ua"] != -7.0).any()
    D.grid_init(g, 1000.0, 1000.0, tmask=user)               # grid_init releases the plan
    assert g._wet is None
