"""GPU tests (-m gpu) of second-order limited tracer transport, dlesm_tracer_step_muscl_f64 / dlesm_tracer_step_muscl_dm
(DESIGN.md section 6.11): bit for bit tests/tracer_muscl_numpy.py on whole arrays -- box, ring and padding of sentinel-filled
outputs.  The sizes are the smallest that cross what can break: 260 x 9 spans three wave tiles of 62 chunks (124 columns)
with both seams, columns 124 and 248, inside the box; 130 x 6 two; 64 x 5 one; 131 x 7 is the odd pitch that takes the
one-cell-per-thread kernel; boxes start on even and on odd columns, hug the array's edge on all four sides (rows j-2 / j+2
and columns i-2 / i+2 then fall outside the array, and the random masks put wet cells into the ring), and shrink to one row
and to one column; 1..8 tracers cover the four instantiations and the two-launch calls.  The HOOK key, an unaligned base and
land fills of NaN and 1e300 give the same bits; an empty box writes nothing.  Wide rows: a row of the box takes
nxw = (x1 / 2 - c_first + 62) / 62 tiles (0-based x1, c_first = (x0 / 2) & ~7), which the launcher's block shape -- four waves
a workgroup, the smallest count that is +-1 modulo 32 -- pads with idle tiles: 260 x 9 has 3 real tiles of 31, 1000 x 9 has 9 of
31 (its real tiles span three workgroups), the sub-box of 1300 x 8 starts mid-row at c_first = 144 and has 9 of 31, 4100 x 7
has 34 of 63; the j5_* shape keys, which reach this launch, change no bit.  Tall boxes: 4200 rows make the second trip of the
one-cell-per-thread kernel's row loop (gridDim.y = 4096), at an even and an odd pitch, and the tile sees the same height.  The
distributed form in loop-back on one GPU
(rank 0 its own eight neighbours through depth-2 tables) equals the single-domain entry followed by the multi-field
exchange, a depth-1 plan is refused, and a plan without messages is the single-domain entry."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

import tracer_cases as TC
import tracer_muscl_numpy as TM
import tracer_numpy as TN
from nemolite_boxes import _dev

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


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
    return None if t is None else C.c_void_p(t.data_ptr())


def _ptrs(ts):
    return (C.c_void_p * max(len(ts), 1))(*[t.data_ptr() for t in ts])


def _hook(D, value):
    D._cabi.lib().dlesm_set_tuning(b"tracer_muscl_kernel", value)


def _call(D, ld, ny, box, tmd, dev, ci, co, entry="dlesm_tracer_step_muscl_f64", plan=None):
    fn = getattr(D._cabi.lib(), entry)
    head = () if plan is None else (plan,)
    return fn(*head, TC.RDT, ld, ny, *box, _p(tmd), _p(dev["area_t"]), *[_p(dev[n]) for n in TC.FLOW], _ptrs(ci), _ptrs(co),
              len(ci), None)


_HOST = {}


def _host(ld, ny, k, seed):
    """host inputs and nothing else, made once per (ld, ny, k, seed) and never modified"""
    key = (ld, ny, k, seed)
    if key not in _HOST:
        rng = np.random.default_rng(seed)
        tm = TC.random_mask(rng, ny, ld)
        area_t, H = TC.flow_inputs(rng, tm)
        c_in, c_out = TC.tracers(rng, tm.shape, k)
        _HOST[key] = (tm, area_t, H, c_in, c_out)
    return _HOST[key]


def _reference(box, tm, area_t, H, c_in, c_out):
    want = [a.copy() for a in c_out]
    TM.tracer_step_muscl(TC.RDT, box, tm, area_t, *[H[n] for n in TC.FLOW], c_in, want)
    return want


def _run(D, ld, ny, box, k, kernel, seed, shift=0, fill=None):
    """one call on device copies of the host case (fill: the tracers' land cells overwritten with it and un / vn with NaN on
    every face that touches land); returns (tm, host inputs used, outputs)"""
    import torch
    tm, area_t, H, c_in, c_out = _host(ld, ny, k, seed)
    if fill is not None:
        H, c_in = TC.overwrite_land(tm, H, c_in, fill)
    dev = _dev(torch, {"area_t": area_t, **H}, shift)
    ci = list(_dev(torch, {str(n): a for n, a in enumerate(c_in)}, shift).values())
    co = list(_dev(torch, {str(n): a for n, a in enumerate(c_out)}, shift).values())
    tmd = torch.from_numpy(tm).cuda()
    try:
        _hook(D, kernel)
        rc = _call(D, ld, ny, box, tmd, dev, ci, co)
        assert rc == 0, D._cabi.lib().dlesm_last_error()
        torch.cuda.synchronize()
    finally:
        _hook(D, 0)
    for n in range(k):
        assert TN.same(ci[n].cpu().numpy(), c_in[n]), n
    for n in TC.FLOW:
        assert TN.same(dev[n].cpu().numpy(), H[n]), n
    assert np.array_equal(tmd.cpu().numpy(), tm)
    return tm, (area_t, H, c_in, c_out), [t.cpu().numpy() for t in co]


def _check(D, ld, ny, box, k, kernel, seed, shift=0):
    tm, (area_t, H, c_in, c_out), got = _run(D, ld, ny, box, k, kernel, seed, shift)
    want = _reference(box, tm, area_t, H, c_in, c_out)
    for n in range(k):
        assert TN.same(got[n], want[n]), (n, np.argwhere(got[n] != want[n])[:8])
    return tm, got


def _edge_box(ld, ny):
    return (2, ld - 1, 2, ny - 1)


BOXES = [
    (260, 9, (2, 259, 2, 8)),        # the ring is the array's edge on all four sides; three tiles, both seams in the box
    (260, 9, (3, 258, 3, 7)),        # starts on an even 0-based column, two cells from every edge
    (260, 9, (124, 250, 4, 6)),      # starts one column before the first seam (odd 0-based), ends beyond the second
    (260, 9, (2, 259, 5, 5)),        # one row
    (260, 9, (125, 125, 2, 8)),      # one column: the first of the second tile
    (260, 9, (124, 124, 2, 8)),      # one column: the last of the first tile
    (130, 6, (2, 129, 2, 5)),
    (130, 6, (5, 126, 3, 4)),
    (64, 5, (2, 63, 2, 4)),
    (64, 5, (2, 2, 2, 4)),           # one column beside the array's west edge
    (64, 5, (63, 63, 2, 4)),         # ... and beside its east edge
    (131, 7, (2, 130, 2, 6)),        # an odd pitch: one cell per thread
    (131, 7, (3, 129, 4, 4)),
    (1000, 9, (2, 999, 2, 8)),       # nxw = (499 - 0 + 62) / 62 = 9 real tiles, padded to 31: three workgroups hold real tiles
    (1300, 8, (301, 1291, 3, 6)),    # starts mid-row: c_first = 150 & ~7 = 144, nxw = (645 - 144 + 62) / 62 = 9, padded to 31
    (4100, 7, (2, 4099, 2, 6)),      # nxw = (2049 + 62) / 62 = 34 real tiles, padded to 63
]
# 4200 rows: the second trip of the one-cell-per-thread kernel's row loop (kernel = 1; 13 is an odd pitch, which takes that
# kernel with kernel = 0), and the tile at the same height
TALL = [(12, 4200, 1), (13, 4200, 0), (66, 4200, 0)]
SHAPE_KEYS = {"j5_autoshape": 1, "j5_tpb": 0, "j5_pad_tiles": 0}       # the keys test_shape_keys_change_no_bit sets: defaults


@pytest.mark.parametrize("ld,ny,box", BOXES)
@pytest.mark.parametrize("kernel", [0, 1])
def test_boxes_and_paths(D, ld, ny, box, kernel):
    """random -1/0/1 masks with wet ring cells, non-uniform metrics, two tracers; kernel = 1: the HOOK key forces the
    one-cell-per-thread kernel, which must leave the same bits (both are compared with the one restatement)"""
    tm, got = _check(D, ld, ny, box, 2, kernel, ld * 7 + ny)
    edge = np.concatenate([tm[0], tm[-1], tm[:, 0], tm[:, -1]])
    assert (edge > 0).any()
    xs, xe, ys, ye = box
    assert (got[0][ys - 1:ye, xs - 1:xe] != TC.SENTINEL).any()


@pytest.mark.parametrize("ld,ny,kernel", TALL)
def test_tall_boxes(D, ld, ny, kernel):
    """two tracers against the array restatement; wet cells were written beyond row 4096 of the box"""
    tm, got = _check(D, ld, ny, _edge_box(ld, ny), 2, kernel, ld * 7 + ny)
    far = tm[4097:ny - 1, 1:ld - 1] > 0              # the box starts at row 1 (0-based): its rows 4096 ..
    assert far.sum() > ld and all((g[4097:ny - 1, 1:ld - 1][far] != TC.SENTINEL).all() for g in got)


def test_shape_keys_change_no_bit(D):
    """1000 x 9, three tracers: the j5_* keys of choose_block_shape reach the tile's launch -- no padding (9 tiles), 2 waves a
    workgroup (15 tiles), 8 and 16 (62 and 124 tiles; the launcher then clamps the workgroup to 4 waves), three tiles more (34)
    -- and every call leaves the restatement's bits; every key is back at its default afterwards"""
    ld, ny = 1000, 9
    box = _edge_box(ld, ny)
    L = D._cabi.lib()
    try:
        for key, value in ((None, 0), ("j5_autoshape", 0), ("j5_tpb", 2), ("j5_tpb", 8), ("j5_tpb", 16), ("j5_pad_tiles", 3)):
            for name, default in SHAPE_KEYS.items():
                L.dlesm_set_tuning(name.encode(), value if name == key else default)
            _check(D, ld, ny, box, 3, 0, ld * 7 + ny)
    finally:
        for name, default in SHAPE_KEYS.items():
            L.dlesm_set_tuning(name.encode(), default)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6, 7, 8])
@pytest.mark.parametrize("ld,ny,kernel", [(260, 9, 0), (131, 7, 0), (130, 6, 1)])
def test_tracer_counts(D, ld, ny, kernel, k):
    """every instantiation (1..4 tracers a launch) and the two-launch calls (5..8); the tracers hold different data, so a
    swapped pointer shows"""
    _check(D, ld, ny, _edge_box(ld, ny), k, kernel, 1000 + ld + k)


@pytest.mark.parametrize("ld,ny,box", [(260, 9, (2, 259, 2, 8)), (130, 6, (5, 126, 3, 4)), (64, 5, (2, 63, 2, 4))])
def test_an_unaligned_base_gives_the_same_bits(D, ld, ny, box):
    """bases 8 bytes off a 16-byte boundary take the one-cell-per-thread kernel: the bits of the aligned call"""
    _, got0 = _check(D, ld, ny, box, 3, 0, 31 + ld, shift=0)
    _, got1 = _check(D, ld, ny, box, 3, 0, 31 + ld, shift=1)
    for a, b in zip(got0, got1):
        assert TN.same(a, b)


@pytest.mark.parametrize("fill", [np.nan, 1e300])
@pytest.mark.parametrize("ld,ny,kernel", [(260, 9, 0), (260, 9, 1), (131, 7, 0), (64, 5, 0)])
def test_land_fills_give_the_same_bits(D, ld, ny, kernel, fill):
    """every tracer's land cells hold `fill` -- cells of the array's edge, two away from a written cell, among them -- and
    un / vn NaN on every face that touches land: every output equals the run without the overwrites, in every cell"""
    box = _edge_box(ld, ny)
    tm, (area_t, H, c_in, c_out), clean = _run(D, ld, ny, box, 2, kernel, 77 + ld)
    _, (_, H2, c2, _), dirty = _run(D, ld, ny, box, 2, kernel, 77 + ld, fill=fill)
    assert (tm == 0).sum() > ld // 4 and np.isnan(H2["un"]).any() and np.isnan(H2["vn"]).any()
    assert not TN.same(c2[0], c_in[0])
    want = _reference(box, tm, area_t, H, c_in, c_out)
    for n in range(2):
        assert TN.same(dirty[n], clean[n]), (n, np.argwhere(dirty[n] != clean[n])[:8])
        assert TN.same(clean[n], want[n]), n
        assert np.isfinite(clean[n][tm > 0]).all()


def test_a_constant_tracer_gets_the_upwind_entrys_bits(D):
    """c = 2.5 everywhere: dlesm_tracer_step_muscl_f64 leaves the bits dlesm_tracer_step_f64 leaves"""
    import torch
    ld, ny = 260, 9
    box = _edge_box(ld, ny)
    tm, area_t, H, _, c_out = _host(ld, ny, 1, 5)
    dev = _dev(torch, {"area_t": area_t, **H}, 0)
    tmd = torch.from_numpy(tm).cuda()
    ci = [torch.full((ny, ld), 2.5, dtype=torch.float64, device="cuda")]
    outs = []
    for entry in ("dlesm_tracer_step_f64", "dlesm_tracer_step_muscl_f64"):
        co = [torch.from_numpy(c_out[0].copy()).cuda()]
        assert _call(D, ld, ny, box, tmd, dev, ci, co, entry=entry) == 0, D._cabi.lib().dlesm_last_error()
        torch.cuda.synchronize()
        outs.append(co[0].cpu().numpy())
    assert TN.same(outs[0], outs[1]) and (outs[0] != TC.SENTINEL).any()


@pytest.mark.parametrize("kernel", [0, 1])
def test_an_empty_box_writes_nothing(D, kernel):
    for ld, ny, box in ((260, 9, (5, 4, 2, 8)), (260, 9, (2, 259, 6, 5)), (131, 7, (9, 8, 2, 6))):
        _, got = _check(D, ld, ny, box, 2, kernel, 3)
        assert all((g == TC.SENTINEL).all() for g in got)


def test_refusals_write_nothing(D):
    """the refusals of section 6.10 through the new entry: DLESM_EINVAL before anything is launched"""
    import torch
    ld, ny = 64, 8
    box = _edge_box(ld, ny)
    tm, area_t, H, c_in, c_out = _host(ld, ny, 2, 9)
    dev = _dev(torch, {"area_t": area_t, **H}, 0)
    tmd = torch.from_numpy(tm).cuda()
    ci = [torch.from_numpy(a).cuda() for a in c_in]
    co = [torch.from_numpy(a.copy()).cuda() for a in c_out]
    L = D._cabi.lib()

    def call(box=box, ci=ci, co=co, k=None, dev=dev):
        return L.dlesm_tracer_step_muscl_f64(TC.RDT, ld, ny, *box, _p(tmd), _p(dev["area_t"]), *[_p(dev[n]) for n in TC.FLOW],
                                             _ptrs(ci), _ptrs(co), len(ci) if k is None else k, None)

    cases = {"k=0": call(k=0), "k=9": call(k=9), "out is in": call(co=[ci[0], co[1]]), "out twice": call(co=[co[0], co[0]]),
             "out is ssha": call(co=[dev["ssha"], co[1]]), "no west ring": call(box=(1, ld - 1, 2, ny - 1)),
             "no east ring": call(box=(2, ld, 2, ny - 1)), "no south ring": call(box=(2, ld - 1, 1, ny - 1)),
             "no north ring": call(box=(2, ld - 1, 2, ny)), "null vn": call(dev={**dev, "vn": None})}
    assert all(rc == D._cabi.EINVAL for rc in cases.values()), cases
    assert b"dlesm_tracer_step_muscl_f64" in L.dlesm_last_error()
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == TC.SENTINEL).all() for t in co)


# ---- the distributed form, in loop-back ---------------------------------------------------------------------------------
class Loop:
    """raw (ny, ld) device arrays, a box with a two-cell ring and a depth-`depth` loop-back plan over it"""

    def __init__(self, D, ld, ny, k, seed, depth=2, peer=0, tables=True, shift=0):
        import torch
        from dm_overhead import loopback_tables
        self.D, self.L = D, D._cabi.lib()
        self.ld, self.ny, self.k = ld, ny, k
        self.box = (3, ld - 2, 3, ny - 2)
        self.tm, self.area_t, self.H, self.c_in, self.c_out = _host(ld, ny, k, seed)
        self.t = loopback_tables(D, D._cabi.Region(ld - 4, ny - 4, *self.box), depth) if tables else D._cabi.CommTables()
        self.dev = _dev(torch, {"area_t": self.area_t, **self.H}, shift)
        self.tmd = torch.from_numpy(self.tm).cuda()
        self.ci = list(_dev(torch, {str(n): a for n, a in enumerate(self.c_in)}, shift).values())
        self.shift = shift
        self.plan = C.c_void_p()
        D._cabi.check(self.L.dlesm_halo_plan_create(C.byref(self.t), ld, ny, C.byref(self.plan)))
        if peer:
            from dl_esm_inf_amd import grid_mod
            grid_mod.connect_peers(types.SimpleNamespace(_halo_plan=self.plan), peer)
            self.L.dlesm_set_tuning(b"dm_skip_parts", 1)      # no RCCL group: only the mailboxes can move the halos

    def outputs(self):
        import torch
        return list(_dev(torch, {str(n): a for n, a in enumerate(self.c_out)}, self.shift).values())

    def single(self, co):
        return _call(self.D, self.ld, self.ny, self.box, self.tmd, self.dev, self.ci, co)

    def one_call(self, co, plan=None):
        return _call(self.D, self.ld, self.ny, self.box, self.tmd, self.dev, self.ci, co, entry="dlesm_tracer_step_muscl_dm",
                     plan=self.plan if plan is None else plan)

    def close(self):
        self.L.dlesm_set_tuning(b"dm_skip_parts", 0)
        _hook(self.D, 0)
        self.D._cabi.check(self.L.dlesm_halo_plan_destroy(self.plan))


@pytest.mark.parametrize("peer", [0, 3])
@pytest.mark.parametrize("ld,ny,k,kernel", [(260, 10, 1, 0), (260, 10, 4, 0), (131, 9, 3, 0), (130, 9, 2, 1), (64, 9, 5, 0)])
def test_one_call_equals_the_definition(D, ld, ny, k, kernel, peer):
    """whole sentinel-filled arrays: every cell of every new tracer equals dlesm_tracer_step_muscl_f64 followed by
    dlesm_halo_exchange_multi_f64 on the same depth-2 plan; peer = 3: the mailboxes connected for three fields (four and
    five tracers: two turns), the RCCL group switched off"""
    import torch
    S = Loop(D, ld, ny, k, ld * 31 + ny + k, peer=peer)
    try:
        _hook(D, kernel)
        Od, O1 = S.outputs(), S.outputs()
        assert S.single(Od) == 0, S.L.dlesm_last_error()
        turn = peer or k
        for n in range(0, k, turn):
            D._cabi.check(S.L.dlesm_halo_exchange_multi_f64(S.plan, _ptrs(Od[n:n + turn]), len(Od[n:n + turn]),
                                                            D._cabi.DIRS_ALL, None))
        assert S.one_call(O1) == 0, S.L.dlesm_last_error()
        torch.cuda.synchronize()
        assert S.L.dlesm_wait_timed_out(0) == 0
        want = _reference(S.box, S.tm, S.area_t, S.H, S.c_in, S.c_out)
        for n in range(k):
            got, dfn = O1[n].cpu().numpy(), Od[n].cpu().numpy()
            assert TN.same(got, dfn), (n, np.argwhere(got != dfn)[:5])
            assert TN.same(got[2:-2, 2:-2], want[n][2:-2, 2:-2]), n
            # the depth-2 halos moved: the two east halo columns hold the two west internal columns (loop-back)
            assert TN.same(got[2:-2, ld - 2:], got[2:-2, 2:4]) and TN.same(got[ny - 2:, 2:-2], got[2:4, 2:-2])
            assert TN.same(S.ci[n].cpu().numpy(), S.c_in[n])
    finally:
        S.close()


@pytest.mark.parametrize("k", [1, 5])
def test_plan_without_messages_is_the_single_domain_call(D, k):
    import torch
    S = Loop(D, 260, 10, k, 4242, tables=False)
    try:
        Os, O1 = S.outputs(), S.outputs()
        assert S.single(Os) == 0 and S.one_call(O1) == 0, S.L.dlesm_last_error()
        torch.cuda.synchronize()
        for n in range(k):
            assert TN.same(O1[n].cpu().numpy(), Os[n].cpu().numpy()), n
            assert (O1[n].cpu().numpy() != TC.SENTINEL).any()
    finally:
        S.close()


def test_dm_refusals(D):
    """a depth-1 plan with messages, a null plan, a plan of other extents, and a refusal of the single-domain entry through
    the distributed one: DLESM_EINVAL before anything is launched or exchanged -- every output untouched"""
    import torch
    from dm_overhead import loopback_tables
    S = Loop(D, 64, 12, 2, 5)
    L = S.L
    t1 = loopback_tables(D, D._cabi.Region(62, 10, 2, 63, 2, 11), 1)
    plan1, plan3 = C.c_void_p(), C.c_void_p()
    D._cabi.check(L.dlesm_halo_plan_create(C.byref(t1), 64, 12, C.byref(plan1)))
    D._cabi.check(L.dlesm_halo_plan_create(C.byref(S.t), 66, 12, C.byref(plan3)))
    try:
        co = S.outputs()
        got = []
        for plan, msg in ((plan1, b"depth-1"), (C.c_void_p(0), b"null plan"), (plan3, b"66x12")):
            rc = S.one_call(co, plan=plan)
            got.append((rc, msg in L.dlesm_last_error(), L.dlesm_last_error()))
        rc = S.one_call([co[0], co[0]])
        got.append((rc, b"overlap" in L.dlesm_last_error(), L.dlesm_last_error()))
        assert all(rc == D._cabi.EINVAL and ok for rc, ok, _ in got), got
        torch.cuda.synchronize()
        for n in range(2):
            assert (co[n].cpu().numpy() == TC.SENTINEL).all() and TN.same(S.ci[n].cpu().numpy(), S.c_in[n])
    finally:
        S.close()
        L.dlesm_halo_plan_destroy(plan1)
        L.dlesm_halo_plan_destroy(plan3)


# ---- through the Python wrappers ----------------------------------------------------------------------------------------
def _pygrid(D, nx, ny, halo_width, ndomains=None):
    import torch
    os.environ["DL_ESM_ALIGNMENT"] = "64"
    try:
        g = D.grid_type(D.GO_ARAKAWA_C, (1, 1, 2), D.GO_OFFSET_NE)
        if ndomains is None:
            g.decompose(nx, ny, halo_width=halo_width)
        else:
            g.decompose(nx, ny, ndomains=ndomains)
        D.grid_init(g, 1000.0, 1000.0)
    finally:
        os.environ.pop("DL_ESM_ALIGNMENT", None)
    rng = np.random.default_rng(nx + ny)
    T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
    pts = {"ssha": T, "un": U, "vn": V, "ht": T, "hu": U, "hv": V, "sshn_t": T, "sshn_u": U, "sshn_v": V}
    H = {n: (10.0 + rng.random((g.ny, g.nx)) if n in ("ht", "hu", "hv") else 0.1 * rng.normal(size=(g.ny, g.nx))) for n in pts}
    F = {}
    for n, p in pts.items():
        F[n] = D.r2d_field(g, p)
        F[n].data.copy_(torch.from_numpy(H[n]))
    c = [1.0 + n + rng.random((g.ny, g.nx)) for n in range(3)]

    def tracers(arrays):
        out = []
        for a in arrays:
            f = D.r2d_field(g, T)
            f.data.copy_(torch.from_numpy(a))
            out.append(f)
        return out
    return g, H, [F[n] for n in pts], c, tracers


def test_python_wrappers(D):
    """invoke_tracer_step_muscl equals the restatement on the grid's own mask and box; on a one-rank grid decomposed with
    halo_width = 2 invoke_tracer_step_muscl_dm is invoke_tracer_step_muscl; on a halo_width = 1 grid it stops, and
    invoke_tracer_step_muscl stops on a decomposed grid and names the distributed wrapper; nothing is written then"""
    import torch
    g, H, F, c, tracers = _pygrid(D, 200, 12, 2)
    Ci = tracers(c)
    sent = [np.full_like(a, TC.SENTINEL) for a in c]
    Co1, Co2 = tracers(sent), tracers(sent)
    D.psy.invoke_tracer_step_muscl(TC.RDT, Co1, Ci, *F)
    D.psy.invoke_tracer_step_muscl_dm(TC.RDT, Co2, Ci, *F)
    torch.cuda.synchronize()
    want = [a.copy() for a in sent]
    TM.tracer_step_muscl(TC.RDT, Co1[0].internal.box(), g.tmask_device.cpu().numpy(), g.area_t_device.cpu().numpy(),
                         H["un"], H["vn"], H["hu"], H["hv"], H["ht"], H["sshn_t"], H["sshn_u"], H["sshn_v"], H["ssha"], c, want)
    for n in range(3):
        assert TN.same(Co1[n].get_data(), want[n]), n
        assert TN.same(Co2[n].get_data(), Co1[n].get_data()), n
        assert (want[n] != TC.SENTINEL).any()
    g1, _, F1, c1, tracers1 = _pygrid(D, 64, 12, 1)
    Ci1, Co1 = tracers1(c1), tracers1([np.full_like(a, TC.SENTINEL) for a in c1])
    with pytest.raises(D._cabi.GoceanStop, match="halo_width 1"):
        D.psy.invoke_tracer_step_muscl_dm(TC.RDT, Co1, Ci1, *F1)
    gd, _, Fd, cd, tracersd = _pygrid(D, 64, 32, 1, ndomains=2)
    Cid, Cod = tracersd(cd), tracersd([np.full_like(a, TC.SENTINEL) for a in cd])
    with pytest.raises(D._cabi.GoceanStop, match="invoke_tracer_step_muscl_dm"):
        D.psy.invoke_tracer_step_muscl(TC.RDT, Cod, Cid, *Fd)
    torch.cuda.synchronize()
    assert all((f.get_data() == TC.SENTINEL).all() for f in Co1 + Cod)
