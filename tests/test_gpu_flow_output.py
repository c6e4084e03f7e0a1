"""GPU tests (-m gpu) of the model's output fields, dlesm_flow_output_f64: every cell of every output
array -- the written ones and the sentinel-filled rest -- equals tests/flow_output_numpy.py bit for bit (any NaN equal to any
NaN), from the wave-tile kernel and from the one-cell-per-thread kernel (HOOK key flow_output_kernel = 1), on the special-value
and the plain case of flow_output_cases at its three shapes -- 260 x 12 spans three wave tiles of 63 chunks with both seams in
the box, 131 x 10 is the odd pitch, 130 x 9 is swept on the sub-box (5, 100, 3, 8) -- in SET and in ADD (twice into the same
arrays with weight 0.375), for all six outputs, each one alone with every unneeded input null, each one alone with every
unneeded input an all-NaN array, and {UT, VT, SPEED}; the inputs are checked unchanged.  With a base shifted by one element; on
one-column and one-row boxes, an empty and an all-land box; on a row of eleven wave tiles; on a tall box whose rows outnumber
the one-cell-per-thread kernel's row strides.  What land holds changes no bit.  Repeats and a second stream give identical
bytes; one capture into a graph replayed twice in ADD mode equals two plain calls.  Every refusal returns DLESM_EINVAL and
leaves the outputs untouched.  The Python wrapper on a one-rank grid.  No tolerance anywhere."""
import ctypes as C
import math

import numpy as np
import pytest

import flow_output_cases as OC
import flow_output_numpy as ON
from flow_output_numpy import same

pytestmark = pytest.mark.gpu
EINVAL = -1             # DLESM_EINVAL
SENTINEL = OC.SENTINEL
KINDS = ["special", "plain"]


@pytest.fixture(scope="module")
def D():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    import dl_esm_inf_amd as d
    torch.cuda.set_device(0)
    d.parallel_init(0, 1, use_rccl=True)
    assert d._cabi.EINVAL == EINVAL
    assert (d._cabi.OUT_SET, d._cabi.OUT_ADD, d._cabi.OUT_COUNT) == (ON.SET, ON.ADD, ON.COUNT)
    return d


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _hook(D, value):
    D._cabi.lib().dlesm_set_tuning(b"flow_output_kernel", value)


def _to_device(a, shift=0):
    """a device copy; shift: the base 8 bytes off a 16-byte boundary"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    if shift:
        t = torch.cat([torch.zeros(1, dtype=t.dtype, device="cuda"), t.flatten()])[1:].view(a.shape)
    return t


def _upload(tm, A, shift=0):
    return _to_device(tm), {n: _to_device(A[n], shift) for n in OC.ARRAYS}


def _ins(dev, sel, nan=None):
    """device pointers of the six inputs: one the selection does not read is null, or the all-NaN array `nan`"""
    need = ON.needs([0 if k in sel else None for k in range(ON.COUNT)])
    return [_p(dev[n]) if need[m] else _p(nan) for m, n in enumerate(OC.ARRAYS)]


def _outs(shape, sel, shift=0, fill=SENTINEL):
    return [_to_device(np.full(shape, fill), shift) if k in sel else None for k in range(ON.COUNT)]


def _call(D, mode, weight, ld, ny, box, tmd, ins, outs, kernel=0, stream=None):
    pout = (C.c_void_p * ON.COUNT)(*[None if o is None else o.data_ptr() for o in outs])
    sp = None if stream is None else C.c_void_p(stream.cuda_stream)
    try:
        _hook(D, kernel)
        return D._cabi.lib().dlesm_flow_output_f64(mode, float(weight), ld, ny, *box, _p(tmd), *ins, pout, sp)
    finally:
        _hook(D, 0)


def _sweep(D, mode, box, tmd, dev, sel, kernel=0, shift=0, nan=None, shape=None):
    """sentinel-filled outputs, one SET call or two ADD calls with OC.WEIGHT; the outputs on the host"""
    import torch
    ny, ld = shape
    outs = _outs(shape, sel, shift)
    for _ in range(2 if mode == ON.ADD else 1):
        rc = _call(D, mode, OC.WEIGHT, ld, ny, box, tmd, _ins(dev, sel, nan), outs, kernel)
        assert rc == 0, D._cabi.lib().dlesm_last_error()
    torch.cuda.synchronize()
    return [None if o is None else o.cpu().numpy() for o in outs]


def _check(got, want, sel, what=None):
    for k in range(ON.COUNT):
        assert (got[k] is None) == (k not in sel)
        if k in sel:
            bad = ~((got[k].view(np.uint64) == want[k].view(np.uint64)) | (np.isnan(got[k]) & np.isnan(want[k])))
            where = np.argwhere(bad)[:6]
            assert same(got[k], want[k]), (what, sel, ON.NAMES[k], int(bad.sum()), where.tolist(),
                                           [(got[k][j, i], want[k][j, i]) for j, i in where])


def _unchanged(tm, A, tmd, dev):
    for n in OC.ARRAYS:
        assert ON.same(dev[n].cpu().numpy(), A[n]) and np.array_equal(
            dev[n].cpu().numpy().view(np.uint64), A[n].view(np.uint64)), n
    assert np.array_equal(tmd.cpu().numpy(), tm)


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("mode", [ON.SET, ON.ADD])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ld,ny,box", OC.SHAPES)
def test_every_cell_equals_the_restatement(D, ld, ny, box, kind, mode, kernel):
    import torch
    tm, A = OC.host(kind, ld, ny)
    tmd, dev = _upload(tm, A)
    nan = torch.full(tm.shape, math.nan, dtype=torch.float64, device="cuda")
    for sel in OC.SELECTIONS:
        want = OC.reference(kind, ld, ny, box, mode, sel)
        got = _sweep(D, mode, box, tmd, dev, sel, kernel, shape=tm.shape)
        _check(got, want, sel, "null")
        if len(sel) == 1:                                   # the unneeded inputs as all-NaN arrays: the null run's bits
            dirty = _sweep(D, mode, box, tmd, dev, sel, kernel, nan=nan, shape=tm.shape)
            k = sel[0]
            assert np.array_equal(dirty[k].view(np.uint64), got[k].view(np.uint64)), (sel, "nan")
    assert torch.isnan(nan).all().item()
    _unchanged(tm, A, tmd, dev)


@pytest.mark.parametrize("mode", [ON.SET, ON.ADD])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ld,ny,box", OC.SHAPES)
def test_shifted_base(D, ld, ny, box, kind, mode):
    """every double array, the outputs too, 8 bytes off a 16-byte boundary: the one-cell-per-thread kernel without the key"""
    tm, A = OC.host(kind, ld, ny)
    tmd, dev = _upload(tm, A, shift=1)
    assert all(dev[n].data_ptr() % 16 == 8 for n in OC.ARRAYS)
    got = _sweep(D, mode, box, tmd, dev, OC.ALL, 0, shift=1, shape=tm.shape)
    _check(got, OC.reference(kind, ld, ny, box, mode), OC.ALL)
    _unchanged(tm, A, tmd, dev)


SMALL = [(2, 259, 5, 5), (2, 259, 2, 2), (2, 259, 11, 11),                   # one row: middle, first, last
         (127, 127, 2, 11), (126, 126, 2, 11), (2, 2, 2, 11), (259, 259, 2, 11),   # one column: beside the seam, the edges
         (21, 21, 5, 5)]                                                     # one cell


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("box", SMALL)
def test_one_row_and_one_column_boxes(D, box, kernel):
    tm, A = OC.host("special", 260, 12)
    tmd, dev = _upload(tm, A)
    for mode in (ON.SET, ON.ADD):
        got = _sweep(D, mode, box, tmd, dev, OC.ALL, kernel, shape=tm.shape)
        _check(got, OC.reference("special", 260, 12, box, mode), OC.ALL, mode)


@pytest.mark.parametrize("kernel", [0, 1])
def test_empty_and_all_land_boxes(D, kernel):
    """the sentinel is intact; the empty box launches nothing"""
    tm, A = OC.plain_host(130, 9)
    tmd, dev = _upload(tm, A)
    for mode in (ON.SET, ON.ADD):
        for box in [(9, 8, 2, 5), (2, 129, 5, 4)]:
            for o in _sweep(D, mode, box, tmd, dev, OC.ALL, kernel, shape=tm.shape):
                assert (o == SENTINEL).all()
        for value in (0, -1):
            land = _to_device(np.full_like(tm, value))
            for o in _sweep(D, mode, (2, 129, 2, 8), land, dev, OC.ALL, kernel, shape=tm.shape):
                assert (o == SENTINEL).all()


def _big_case(ld, ny):
    rng = np.random.default_rng(ld * 7 + ny)
    import tracer_cases as TC
    tm = TC.random_mask(rng, ny, ld)
    return tm, OC._fields(rng, tm)


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("box", [(2, 1399, 2, 4), (301, 1391, 3, 4)])
def test_wide_row(D, box, kernel):
    """1400 x 5: eleven whole wave tiles a row and the start of a twelfth (padded with idle ones by the launcher's block
    shape), every seam in the box; and a box that starts mid-row"""
    tm, A = _big_case(1400, 5)
    tmd, dev = _upload(tm, A)
    for mode in (ON.SET, ON.ADD):
        want = OC.outputs(tm.shape, OC.ALL)
        for _ in range(2 if mode == ON.ADD else 1):
            ON.flow_output(mode, OC.WEIGHT, box, tm, *[A[n] for n in OC.ARRAYS], want)
        _check(_sweep(D, mode, box, tmd, dev, OC.ALL, kernel, shape=tm.shape), want, OC.ALL, mode)


@pytest.mark.parametrize("ld,ny", [(16, 4200), (4200, 16)])
def test_tall_box_through_the_one_cell_per_thread_kernel(D, ld, ny):
    """16 columns x 4200 rows: more rows than the kernel's 4096 row strides, so its row loop makes a second trip; and 4200
    columns x 16 rows, seventeen workgroups a row"""
    tm, A = _big_case(ld, ny)
    box = (2, ld - 1, 2, ny - 1)
    tmd, dev = _upload(tm, A)
    for mode in (ON.SET, ON.ADD):
        want = OC.outputs(tm.shape, OC.ALL)
        for _ in range(2 if mode == ON.ADD else 1):
            ON.flow_output(mode, OC.WEIGHT, box, tm, *[A[n] for n in OC.ARRAYS], want)
        _check(_sweep(D, mode, box, tmd, dev, OC.ALL, 1, shape=tm.shape), want, OC.ALL, mode)
    assert ON.written(tm, box, ON.VORT)[4100:].any() or ny < 4200


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ld,ny,box", OC.SHAPES)
def test_what_land_holds_changes_no_bit(D, ld, ny, box, kind, kernel):
    """NaN in un / vn on every face that touches land and NaN, an infinity and -3 in ht, sshn_t, dx_v, dy_u of every land cell"""
    tm, A = OC.host(kind, ld, ny)
    A2 = OC.land_overwritten(tm, A)
    tmd, dev = _upload(tm, A2)
    for mode in (ON.SET, ON.ADD):
        _check(_sweep(D, mode, box, tmd, dev, OC.ALL, kernel, shape=tm.shape), OC.reference(kind, ld, ny, box, mode), OC.ALL, mode)
    _unchanged(tm, A2, tmd, dev)


@pytest.mark.parametrize("kernel", [0, 1])
def test_uniform_flow_and_a_mean_of_four_steps(D, kernel):
    """un = a, vn = b on an all-wet patch: UT = a, VT = b, VORT = 0.0 exactly; four ADD calls with weight 1/4 into arrays of
    -0.0 leave SET's bits (test_flow_output_numpy.py says why)"""
    import torch
    ld, ny, box = 260, 12, (2, 259, 2, 11)
    a, b = 0.3, -1.7
    tm, A = OC.plain_host(ld, ny)
    tm1 = np.ones_like(tm)
    A1 = dict(A, un=np.full(tm.shape, a), vn=np.full(tm.shape, b))
    tmd, dev = _upload(tm1, A1)
    got = _sweep(D, ON.SET, box, tmd, dev, OC.ALL, kernel, shape=tm.shape)
    w = ON.written(tm1, box, ON.VORT)
    assert w.sum() == 258 * 10
    assert (got[ON.UT][w] == a).all() and (got[ON.VT][w] == b).all()
    assert (got[ON.VORT][w] == 0.0).all() and not np.signbit(got[ON.VORT][w]).any()
    tmd, dev = _upload(tm, A)
    outs = _outs(tm.shape, OC.ALL, fill=-0.0)
    for _ in range(4):
        assert _call(D, ON.ADD, 0.25, ld, ny, box, tmd, _ins(dev, OC.ALL), outs, kernel) == 0
    torch.cuda.synchronize()
    want = OC.reference("plain", ld, ny, box, ON.SET)
    for k in range(ON.COUNT):
        wk = ON.written(tm, box, k)
        o = outs[k].cpu().numpy()
        assert same(o[wk], want[k][wk]) and np.signbit(o[~wk]).all() and (o[~wk] == 0.0).all(), ON.NAMES[k]


def test_repeats_streams_and_a_graph_give_identical_bytes(D):
    import torch
    ld, ny, box = OC.SHAPES[0]
    tm, A = OC.host("special", ld, ny)
    tmd, dev = _upload(tm, A)
    second = torch.cuda.Stream()
    want = OC.reference("special", ld, ny, box, ON.ADD)
    for kernel in (0, 1):
        for stream in (None, None, second):
            outs = _outs(tm.shape, OC.ALL)
            if stream is not None:
                stream.wait_stream(torch.cuda.current_stream())
            for _ in range(2):
                assert _call(D, ON.ADD, OC.WEIGHT, ld, ny, box, tmd, _ins(dev, OC.ALL), outs, kernel, stream) == 0
            (stream or torch.cuda.current_stream()).synchronize()
            _check([o.cpu().numpy() for o in outs], want, OC.ALL, (kernel, stream is not None))
        # one capture, replayed twice, equals two plain calls
        outs = _outs(tm.shape, OC.ALL)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
            rc = _call(D, ON.ADD, OC.WEIGHT, ld, ny, box, tmd, _ins(dev, OC.ALL), outs, kernel, s)
        assert rc == 0, D._cabi.lib().dlesm_last_error()
        torch.cuda.synchronize()
        assert all((o == SENTINEL).all().item() for o in outs)       # captured, not run
        graph.replay()
        graph.replay()
        torch.cuda.synchronize()
        _check([o.cpu().numpy() for o in outs], want, OC.ALL, (kernel, "graph"))
    _unchanged(tm, A, tmd, dev)


def test_refusals(D):
    """DLESM_EINVAL before anything is launched; the outputs keep their bits"""
    import torch
    L = D._cabi.lib()
    ld, ny, box = 130, 9, (2, 129, 2, 8)
    tm, A = OC.plain_host(ld, ny)
    tmd, dev = _upload(tm, A)
    outs = _outs(tm.shape, OC.ALL)
    ins = _ins(dev, OC.ALL)

    def call(mode=ON.SET, weight=0.5, b=box, mask=None, inputs=None, out=None, sizes=(ld, ny)):
        o = outs if out is None else out
        pout = (C.c_void_p * ON.COUNT)(*[None if x is None else (x if isinstance(x, int) else x.data_ptr()) for x in o])
        rc = L.dlesm_flow_output_f64(mode, float(weight), *sizes, *b, _p(tmd) if mask is None else mask,
                                     *(ins if inputs is None else inputs), pout, None)
        torch.cuda.synchronize()
        assert all((x == SENTINEL).all().item() for x in outs), "an output was written"
        return rc

    for mode in (-1, 2, 7):
        assert call(mode=mode) == EINVAL
    for weight in (math.nan, math.inf, -math.inf):
        assert call(mode=ON.ADD, weight=weight) == EINVAL
    assert call(out=[None] * ON.COUNT) == EINVAL                               # every out entry null
    assert L.dlesm_flow_output_f64(ON.SET, 0.0, ld, ny, *box, _p(tmd), *ins, None, None) == EINVAL
    assert call(mask=C.c_void_p(None)) == EINVAL
    for m in range(6):                                                         # a needed input null / 4 bytes off
        for bad_ptr in (None, C.c_void_p(ins[m].value + 4)):
            bad = list(ins)
            bad[m] = bad_ptr
            assert call(inputs=bad) == EINVAL, m
    # ... while one that no wanted output reads may be null: ht without KE, dx_v / dy_u without VORT
    assert call(mask=C.c_void_p(tmd.data_ptr() + 2)) == EINVAL                 # the mask 2 bytes off
    for k in range(ON.COUNT):                                                  # an output 4 bytes off
        bad = list(outs)
        bad[k] = outs[k].data_ptr() + 4
        assert call(out=bad) == EINVAL, k
    for b in [(1, 129, 2, 8), (2, 130, 2, 8), (2, 129, 1, 8), (2, 129, 2, 9), (0, 5, 2, 8), (2, 131, 2, 8)]:
        assert call(b=b) == EINVAL, b                                          # a box without its ring
    assert call(sizes=(0, ny)) == EINVAL and call(sizes=(ld, 0)) == EINVAL
    for k in range(ON.COUNT):                                                  # an output that overlaps an input ...
        for m, n in enumerate(OC.ARRAYS):
            bad = list(outs)
            bad[k] = dev[n].data_ptr() + 8 * (ld * (ny - 1))                   # (its last row)
            assert call(out=bad) == EINVAL, (k, n)
        bad = list(outs)
        bad[k] = tmd.data_ptr() + 8 * 16                                       # ... the mask ...
        assert call(out=bad) == EINVAL, k
        for m in range(ON.COUNT):                                              # ... or another output
            if m != k:
                bad = list(outs)
                bad[k] = outs[m].data_ptr() + 8 * ld
                assert call(out=bad) == EINVAL, (k, m)
    _unchanged(tm, A, tmd, dev)
    # weight is ignored by SET, and what was refused above still works
    for weight in (math.nan, math.inf):
        assert call(mode=ON.SET, weight=weight, out=[None] * 5 + [_outs(tm.shape, (5,))[5]]) == 0
    rc = L.dlesm_flow_output_f64(ON.SET, math.nan, ld, ny, *box, _p(tmd), *ins,
                                 (C.c_void_p * ON.COUNT)(*[o.data_ptr() for o in outs]), None)
    torch.cuda.synchronize()
    assert rc == 0
    _check([o.cpu().numpy() for o in outs], OC.reference("plain", ld, ny, box, ON.SET), OC.ALL)


def _grid_case(D, nx, ny, alignment):
    """a one-rank grid with a -1/0/1 user mask and hashed flow fields (test_gpu_flow_courant.py's inputs)"""
    import os
    os.environ["DL_ESM_ALIGNMENT"] = str(alignment)
    try:
        g = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
        g.decompose(nx, ny)
        it = g.subdomain.internal
        jj, ii = np.mgrid[1:it.ystop + 2, 1:it.xstop + 2]
        user = ((7 * ii + 13 * jj + (ii * jj) // 5) % 3 - 1).astype(np.int32)
        user[:3, :3] = 0
        D.grid_init(g, 1000.0, 1000.0, tmask=user)
    finally:
        os.environ.pop("DL_ESM_ALIGNMENT", None)
    T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
    F, H = {}, {}
    for k, (name, pt) in enumerate(zip(("un", "vn", "ht", "sshn_t"), (U, V, T, T)), start=2):
        f = D.r2d_field(g, pt)
        D.psy.hash_init(f, 500 + k)
        d = f.get_data()
        d = 0.4 * d - 0.2 if k in (2, 3) else 10.0 + d if k == 4 else 0.05 * d
        f.set_data(d)
        F[name], H[name] = f, np.ascontiguousarray(d)
    return g, F, H


@pytest.mark.parametrize("nx,ny,alignment", [(257, 6, 2), (128, 4, 1)])
def test_python_wrapper(D, nx, ny, alignment):
    """psy.flow_output on a one-rank grid: the restatement's arrays over the T internal region with the grid's mask, dx_v and
    dy_u; weight = None is SET, a number ADD; a selection leaves the other fields alone and needs no ht; halos untouched"""
    g, F, H = _grid_case(D, nx, ny, alignment)
    tm = g.tmask_device.cpu().numpy()
    dx_v, dy_u = g.dx_v_device.cpu().numpy(), g.dy_u_device.cpu().numpy()
    box = F["sshn_t"].internal.box()
    flow = [F[k] for k in ("un", "vn", "ht", "sshn_t")]
    hflow = [H[k] for k in ("un", "vn", "ht", "sshn_t")]
    fields = []
    for _ in range(ON.COUNT):
        f = D.r2d_field(g, D.GO_T_POINTS)
        f.set_data(np.full((g.ny, g.nx), SENTINEL))
        fields.append(f)
    want = OC.outputs(tm.shape, OC.ALL)
    ON.flow_output(ON.SET, 0.0, box, tm, dx_v, dy_u, *hflow, want)
    D.psy.flow_output(*flow, **dict(zip(ON.NAMES, fields)))
    _check([f.get_data() for f in fields], want, OC.ALL, "set")
    assert (want[ON.VORT] == SENTINEL).sum() > (want[ON.UT] == SENTINEL).sum()
    assert ON.written(tm, box, ON.VORT).sum() >= 10 or ny < 6          # (the four-row grid holds no corner clear of land)
    for _ in range(2):
        ON.flow_output(ON.ADD, 0.375, box, tm, dx_v, dy_u, *hflow, want)
        D.psy.flow_output(*flow, **dict(zip(ON.NAMES, fields)), weight=0.375)
    _check([f.get_data() for f in fields], want, OC.ALL, "add")
    # a selection: the velocities alone, without ht and sshn_t
    before = [f.get_data().copy() for f in fields]
    D.psy.flow_output(F["un"], F["vn"], None, None, ut=fields[ON.UT], vt=fields[ON.VT], speed=fields[ON.SPEED])
    ref = OC.outputs(tm.shape, (ON.UT, ON.VT, ON.SPEED))
    ON.flow_output(ON.SET, 0.0, box, tm, None, None, H["un"], H["vn"], None, None, ref)
    for k in range(ON.COUNT):
        assert same(fields[k].get_data(), ref[k] if ref[k] is not None else before[k]), ON.NAMES[k]
    with pytest.raises(D.DlesmError, match="no output field"):
        D.psy.flow_output(*flow)
    with pytest.raises(D.DlesmError, match="ke needs ht"):
        D.psy.flow_output(F["un"], F["vn"], None, F["sshn_t"], ke=fields[ON.KE])
    with pytest.raises(D.DlesmError, match="T-point fields"):
        D.psy.flow_output(*flow, ut=F["un"])
    assert D.flow_output is D.psy.flow_output
    for name in ("un", "vn", "ht", "sshn_t"):
        assert same(F[name].get_data(), H[name]), name
