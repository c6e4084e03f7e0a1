"""GPU tests (-m gpu) of the flow step's stability check, dlesm_flow_courant_async_f64 / dlesm_flow_courant_f64 (DESIGN.md
section 6.15): every member of the record equals tests/flow_courant_numpy.py, from the wave-tile kernel and from the
one-cell-per-thread kernel (HOOK key flow_courant_kernel = 1), on the special-value and the plain case of flow_courant_cases at
its three shapes -- 260 x 12 spans three wave tiles of 63 chunks with both seams in the box, 131 x 10 is the odd pitch, 130 x 9
is swept on the sub-box (5, 100, 3, 8) -- at two rdt and two sets of limits; with a base shifted by one element; on one-column
and one-row boxes, an empty box and an all-land box; on a tall box whose records need two levels of the reduction (the record
count is asserted on the host); on a wide row of eleven wave tiles.  What land holds changes no member.  Every kind of bad
cell is in the special case (test_flow_courant_numpy.py's census).  A cell at exactly a limit counts, none does one ulp
beyond.  visc == 0.  The asynchronous and the synchronous form, repeats and a second stream give identical bytes.  Every
refusal returns DLESM_EINVAL and leaves result_dev untouched.  The Python wrappers on a one-rank grid.  No tolerance anywhere."""
import ctypes as C
import math

import numpy as np
import pytest

import flow_courant_cases as FC
import flow_courant_numpy as FN
import tracer_courant_numpy as CN
from nemolite_boxes import _dev
from tracer_numpy import same

pytestmark = pytest.mark.gpu
EINVAL = -1             # DLESM_EINVAL
SENTINEL = -7.0
LEVEL_CHUNK = 1024      # records one workgroup of a reduction level combines (dlesm_record_reduce.h)


@pytest.fixture(scope="module")
def D():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    import dl_esm_inf_amd as d
    torch.cuda.set_device(0)
    d.parallel_init(0, 1, use_rccl=True)
    assert d._cabi.EINVAL == EINVAL
    return d


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _hook(D, value):
    D._cabi.lib().dlesm_set_tuning(b"flow_courant_kernel", value)


def _upload(tm, A, shift=0):
    import torch
    return torch.from_numpy(tm).cuda(), _dev(torch, {k: A[k] for k in FC.ARRAYS}, shift)


def _args(rdt, ld, ny, box, tmd, dev, limits, visc=FC.VISC, g=FC.G):
    return (float(rdt), float(g), float(visc), ld, ny, *box, _p(tmd), *[_p(dev[n]) for n in FC.ARRAYS],
            *[float(x) for x in limits])


def _raw(res):
    """the 128 bytes of a device record"""
    return res.cpu().numpy().tobytes()


def _record(raw):
    from dl_esm_inf_amd._cabi import FlowCourant
    r = FlowCourant.from_buffer_copy(raw).as16()
    assert r[14:] == (0, 0)                                # reserved: written as 0
    return FN.Record(*r[:14])


def _device_call(D, rdt, ld, ny, box, tmd, dev, limits=FC.LIMITS, kernel=0, stream=None, sync=False, visc=FC.VISC, raw=False):
    """one call; the asynchronous form into a sentinel-filled device record, or the synchronous one"""
    import torch
    L = D._cabi.lib()
    sp = None if stream is None else C.c_void_p(stream.cuda_stream)
    try:
        _hook(D, kernel)
        if sync:
            out = D._cabi.FlowCourant()
            rc = L.dlesm_flow_courant_f64(*_args(rdt, ld, ny, box, tmd, dev, limits, visc), C.byref(out), sp)
            assert rc == 0, L.dlesm_last_error()
            got = bytes(out)
        else:
            res = torch.full((16,), SENTINEL, dtype=torch.float64, device="cuda")
            if stream is not None:
                stream.wait_stream(torch.cuda.current_stream())
            rc = L.dlesm_flow_courant_async_f64(*_args(rdt, ld, ny, box, tmd, dev, limits, visc), _p(res), sp)
            assert rc == 0, L.dlesm_last_error()
            (stream or torch.cuda.current_stream()).synchronize()
            got = _raw(res)
    finally:
        _hook(D, 0)
    return got if raw else _record(got)


def _run(D, tm, A, rdt, box, kernel=0, shift=0, limits=FC.LIMITS, visc=FC.VISC):
    """upload, call, and check that no input changed"""
    ny, ld = tm.shape
    tmd, dev = _upload(tm, A, shift)
    got = _device_call(D, rdt, ld, ny, box, tmd, dev, limits, kernel, visc=visc)
    for n in FC.ARRAYS:
        assert same(dev[n].cpu().numpy(), A[n]), n
    assert np.array_equal(tmd.cpu().numpy(), tm)
    return got


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("rdt,limits", [(FC.RDT, FC.LIMITS), (FC.RDT_BIG, FC.LIMITS_BIG)])
@pytest.mark.parametrize("kind", ["special", "plain"])
@pytest.mark.parametrize("ld,ny,box", FC.SHAPES)
def test_every_member_equals_the_restatement(D, ld, ny, box, kind, rdt, limits, kernel):
    tm, A = FC.host(kind, ld, ny)
    got = _run(D, tm, A, rdt, box, kernel, limits=limits)
    want = FC.reference(kind, ld, ny, box, rdt, limits)
    print(got)
    assert FN.same_record(got, want), (got, want)


@pytest.mark.parametrize("kind", ["special", "plain"])
@pytest.mark.parametrize("ld,ny,box", FC.SHAPES)
def test_shifted_base(D, ld, ny, box, kind):
    """every double array 8 bytes off a 16-byte boundary: the one-cell-per-thread kernel without the key"""
    tm, A = FC.host(kind, ld, ny)
    got = _run(D, tm, A, FC.RDT_BIG, box, 0, shift=1, limits=FC.LIMITS_BIG)
    assert FN.same_record(got, FC.reference(kind, ld, ny, box, FC.RDT_BIG, FC.LIMITS_BIG)), got


SMALL = [(2, 259, 5, 5), (2, 259, 2, 2), (2, 259, 11, 11),                   # one row: middle, first, last
         (127, 127, 2, 11), (126, 126, 2, 11), (2, 2, 2, 11), (259, 259, 2, 11),   # one column: beside the seam, the edges
         (21, 21, 5, 5)]                                                     # one cell


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("box", SMALL)
def test_one_row_and_one_column_boxes(D, box, kernel):
    tm, A = FC.host("special", 260, 12)
    got = _run(D, tm, A, FC.RDT_BIG, box, kernel, limits=FC.LIMITS_BIG)
    assert FN.same_record(got, FC.reference("special", 260, 12, box, FC.RDT_BIG, FC.LIMITS_BIG)), got


@pytest.mark.parametrize("kernel", [0, 1])
def test_empty_and_all_land_boxes(D, kernel):
    """{0, 0, 0, +inf, -1, -1, -1, -1, 0 ...}; the empty box reads nothing (its arrays' pointers are only checked)"""
    tm, A = FC.plain_host(130, 9)
    for box in [(9, 8, 2, 5), (2, 129, 5, 4)]:
        assert _run(D, tm, A, FC.RDT, box, kernel) == FN.EMPTY
    for value in (0, -1):
        assert _run(D, np.full_like(tm, value), A, FC.RDT, (2, 129, 2, 8), kernel) == FN.EMPTY


def _records(ld, box, kernel):
    """records the sweep leaves = its workgroups, for a box one wave tile wide: the tile form packs four waves, one per row,
    into a workgroup; the one-cell-per-thread form has 256 columns and at most 4096 row strides"""
    xs, xe, ys, ye = box
    h = ye - ys + 1
    if kernel == 0:
        c_first = ((xs - 1) // 2) & ~7
        nxw = ((xe - 1) // 2 - c_first + 63) // 63
        assert nxw == 1                                   # (wider rows get idle padding tiles)
        return (nxw * h + 3) // 4
    return ((xe - xs + 256) // 256) * min(h, 4096)


@pytest.mark.parametrize("kernel", [0, 1])
def test_tall_box_runs_two_levels(D, kernel):
    """66 x 4200 (test_gpu_tracer_courant.py's tall box): 1050 records from the tile form, 4096 from the one-cell-per-thread
    form (whose row loop makes its second trip) -- more than one workgroup of a level holds, so a second level runs; fewer
    than 1024**2, beyond which a third would"""
    ld, ny = 66, 4200
    box = (2, ld - 1, 2, ny - 1)
    n = _records(ld, box, kernel)
    assert n == (1050 if kernel == 0 else 4096) and LEVEL_CHUNK < n <= LEVEL_CHUNK ** 2
    tm, A = FC.plain_host(ld, ny)
    want = FC.reference("plain", ld, ny, box, FC.RDT_BIG, FC.LIMITS_BIG)
    got = _run(D, tm, A, FC.RDT_BIG, box, kernel, limits=FC.LIMITS_BIG)
    assert FN.same_record(got, want), (got, want)
    assert min(want[4:8]) // ld > 0 and want.wet > 100000 and want.gravity_over > 0


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("box", [(2, 1299, 2, 7), (301, 1291, 3, 6)])
def test_wide_row(D, box, kernel):
    """1300 x 8: eleven wave tiles a row (padded with idle ones by the launcher's block shape), every seam in the box; and a
    box that starts mid-row"""
    tm, A = FC.plain_host(1300, 8)
    want = FC.reference("plain", 1300, 8, box, FC.RDT_BIG, FC.LIMITS_BIG)
    got = _run(D, tm, A, FC.RDT_BIG, box, kernel, limits=FC.LIMITS_BIG)
    assert FN.same_record(got, want), (got, want)


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("kind", ["special", "plain"])
@pytest.mark.parametrize("ld,ny,box", FC.SHAPES)
def test_land_changes_no_member(D, ld, ny, box, kind, kernel):
    """NaN in un / vn on every face that touches land and NaN, infinities, negative numbers in ht, sshn_t, dx_t, dy_t on every
    land cell"""
    tm, A = FC.host(kind, ld, ny)
    got = _run(D, tm, FC.land_overwritten(tm, A), FC.RDT_BIG, box, kernel)
    assert FN.same_record(got, FC.reference(kind, ld, ny, box, FC.RDT_BIG)), got


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("kind", ["special", "plain"])
def test_a_cell_at_each_limit_counts(D, kind, kernel):
    """limits equal to the record's own extremes: the cells that hold them count; one ulp beyond, none does"""
    ld, ny, box = FC.SHAPES[0]
    tm, A = FC.host(kind, ld, ny)
    at, beyond = FC.at_the_limits(FC.reference(kind, ld, ny, box, FC.RDT))
    r = _run(D, tm, A, FC.RDT, box, kernel, limits=at)
    assert FN.same_record(r, FN.flow_courant(FC.RDT, FC.G, FC.VISC, box, tm, *FC.arrays(A), *at)), r
    assert min(r.gravity_over, r.advective_over, r.viscous_over, r.shallow) >= 1
    r = _run(D, tm, A, FC.RDT, box, kernel, limits=beyond)
    assert FN.same_record(r, FN.flow_courant(FC.RDT, FC.G, FC.VISC, box, tm, *FC.arrays(A), *beyond)), r
    assert (r.gravity_over, r.advective_over, r.viscous_over, r.shallow) == (0, 0, 0, 0)


@pytest.mark.parametrize("kernel", [0, 1])
def test_no_viscosity(D, kernel):
    ld, ny, box = FC.SHAPES[0]
    for kind in ("special", "plain"):
        tm, A = FC.host(kind, ld, ny)
        r = _run(D, tm, A, FC.RDT_BIG, box, kernel, visc=0.0)
        assert FN.same_record(r, FC.reference(kind, ld, ny, box, FC.RDT_BIG, visc=0.0)), r
        assert r.viscous_max == 0.0 and r.viscous_over == 0 and r.viscous_index >= 0


def test_forms_repeats_and_streams_give_identical_bytes(D):
    import torch
    rdt, (ld, ny, box) = FC.RDT_BIG, FC.SHAPES[0]
    tm, A = FC.host("special", ld, ny)
    want = FC.reference("special", ld, ny, box, rdt, FC.LIMITS_BIG)
    tmd, dev = _upload(tm, A)
    second = torch.cuda.Stream()
    got = []
    for kernel in (0, 1):
        kw = dict(limits=FC.LIMITS_BIG, kernel=kernel, raw=True)
        got += [_device_call(D, rdt, ld, ny, box, tmd, dev, **kw) for _ in range(3)]
        got.append(_device_call(D, rdt, ld, ny, box, tmd, dev, sync=True, **kw))
        got.append(_device_call(D, rdt, ld, ny, box, tmd, dev, stream=second, **kw))
        got.append(_device_call(D, rdt, ld, ny, box, tmd, dev, stream=second, sync=True, **kw))
    assert FN.same_record(_record(got[0]), want), (_record(got[0]), want)
    assert all(len(g) == 128 and g == got[0] for g in got)


def test_refusals(D):
    """DLESM_EINVAL before anything is launched; result_dev keeps its bits"""
    import torch
    L = D._cabi.lib()
    ld, ny, box = 130, 9, (2, 129, 2, 8)
    tm, A = FC.plain_host(ld, ny)
    tmd, dev = _upload(tm, A)
    res = torch.full((16,), SENTINEL, dtype=torch.float64, device="cuda")
    good = list(_args(FC.RDT, ld, ny, box, tmd, dev, FC.LIMITS))
    before = (1.0, 2.0, 3.0, 4.0, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14)

    def refused(args, stream=None):
        rc = L.dlesm_flow_courant_async_f64(*args, _p(res), stream)
        host = D._cabi.FlowCourant(*before[:14], before[14:])
        rc2 = L.dlesm_flow_courant_f64(*args, C.byref(host), stream)
        torch.cuda.synchronize()
        return rc == EINVAL and rc2 == EINVAL and (res == SENTINEL).all().item() and host.as16() == before

    assert L.dlesm_flow_courant_async_f64(*good, _p(res), None) == 0
    torch.cuda.synchronize()
    assert (res != SENTINEL).all().item()
    res.fill_(SENTINEL)
    for k in range(9, 16):                                                     # a null pointer: tmask .. sshn_t
        bad = list(good)
        bad[k] = None
        assert refused(bad), k
    assert L.dlesm_flow_courant_async_f64(*good, None, None) == EINVAL
    assert L.dlesm_flow_courant_f64(*good, None, None) == EINVAL
    for k in range(10, 16):                                                    # a double array 4 bytes off
        bad = list(good)
        bad[k] = C.c_void_p(good[k].value + 4)
        assert refused(bad), k
    bad = list(good)
    bad[9] = C.c_void_p(good[9].value + 2)                                     # the mask 2 bytes off
    assert refused(bad)
    for b in [(1, 129, 2, 8), (2, 130, 2, 8), (2, 129, 1, 8), (2, 129, 2, 9), (0, 5, 2, 8), (2, 131, 2, 8)]:
        bad = list(good)                                                       # a box without its ring
        bad[5:9] = b
        assert refused(bad), b
    for value in (math.nan, 0.0, -0.0, -1.0, -math.inf):                       # rdt, g and the three number limits: > 0
        for k in (0, 1, 16, 17, 18):
            bad = list(good)
            bad[k] = value
            assert refused(bad), (k, value)
    for value in (math.nan, -1.0, -math.inf, -5e-324):                         # visc and depth_limit: >= 0
        for k in (2, 19):
            bad = list(good)
            bad[k] = value
            assert refused(bad), (k, value)
    for name in FC.ARRAYS:                                                     # result_dev inside an input array
        t = dev[name]
        rc = L.dlesm_flow_courant_async_f64(*good, C.c_void_p(t.data_ptr() + 8 * (ld * ny - 16)), None)
        torch.cuda.synchronize()
        assert rc == EINVAL and same(t.cpu().numpy(), A[name]), name
    rc = L.dlesm_flow_courant_async_f64(*good, C.c_void_p(tmd.data_ptr() + 4 * (ld * ny - 32)), None)
    assert rc == EINVAL and np.array_equal(tmd.cpu().numpy(), tm)
    # under stream capture the call is refused before it enqueues anything: the capture stays intact and replays
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    x = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        x.add_(1.0)
        rc = L.dlesm_flow_courant_async_f64(*good, _p(res), sp)
        host = D._cabi.FlowCourant(*before[:14], before[14:])
        rc2 = L.dlesm_flow_courant_f64(*good, C.byref(host), sp)
    assert rc == EINVAL and rc2 == EINVAL and host.as16() == before
    graph.replay()
    torch.cuda.synchronize()
    assert (x == 1.0).all().item() and (res == SENTINEL).all().item()
    # and the arguments that were refused above still work; zero is a valid visc and depth_limit
    assert L.dlesm_flow_courant_async_f64(*good, _p(res), None) == 0
    torch.cuda.synchronize()
    assert FN.same_record(_record(_raw(res)), FC.reference("plain", ld, ny, box, FC.RDT))


def _grid_case(D, nx, ny, alignment):
    """a one-rank grid with a -1/0/1 user mask and hashed flow fields (test_gpu_tracer_courant.py's inputs)"""
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
    names = ("un", "vn", "ht", "hu", "hv", "sshn_t", "sshn_u", "sshn_v")                 # tracer_courant's order
    for k, (name, pt) in enumerate(zip(names, (U, V, T, U, V, T, U, V)), start=2):
        f = D.r2d_field(g, pt)
        D.psy.hash_init(f, 500 + k)
        d = f.get_data()
        d = 0.4 * d - 0.2 if k in (2, 3) else 10.0 + d if k in (4, 5, 6) else 0.05 * d
        f.set_data(d)
        F[name], H[name] = f, np.ascontiguousarray(d)
    return g, F, H


def _at(g, index):
    return (1, index % g.nx + 1, index // g.nx + 1)


@pytest.mark.parametrize("nx,ny,alignment", [(257, 6, 2), (128, 4, 1)])
def test_python_wrappers(D, nx, ny, alignment):
    """psy.flow_courant on arrays (260, 9) and (131, 7): the restatement's record, locations as (rank, i, j), the estimate of
    rdt; psy.flow_courant_check raises on each of the counts and returns the result otherwise; psy.step_rdt_limit is the
    smaller of the two restatements' estimates"""
    g, F, H = _grid_case(D, nx, ny, alignment)
    tm = g.tmask_device.cpu().numpy()
    dx_t, dy_t = g.dx_t_device.cpu().numpy(), g.dy_t_device.cpu().numpy()
    area_t = g.area_t_device.cpu().numpy()
    flow = [F[k] for k in ("un", "vn", "ht", "sshn_t")]
    hflow = [H[k] for k in ("un", "vn", "ht", "sshn_t")]
    box = F["sshn_t"].internal.box()
    params = D.psy.momentum_params(70.0, 0.00015, FC.VISC, FC.G)
    for rdt in (70.0, 20.0):
        want = FN.flow_courant(rdt, FC.G, FC.VISC, box, tm, dx_t, dy_t, *hflow)
        r = D.psy.flow_courant(rdt, *flow, g=FC.G, visc=FC.VISC)
        print(r)
        assert r == D.psy.flow_courant(rdt, *flow, params=params)
        assert tuple(r[:4]) == tuple(want[:4]) and tuple(r[8:14]) == tuple(want[8:14])
        assert tuple(r[4:8]) == tuple(_at(g, i) for i in want[4:8])
        assert r.rdt_limit == FN.rdt_limit(rdt, want) and 0.0 < r.rdt_limit < math.inf
        # the one call of an adaptive loop: the smaller of the flow's and the tracers' estimate
        tracer = CN.tracer_courant(rdt, box, tm, area_t, *[H[k] for k in ("un", "vn", "hu", "hv", "ht", "sshn_t", "sshn_u",
                                                                           "sshn_v")])
        both = D.psy.step_rdt_limit(rdt, *F.values(), params=params)
        assert both == min(FN.rdt_limit(rdt, want), CN.rdt_limit(rdt, tracer))
        assert FN.flow_courant_scalar(rdt, FC.G, FC.VISC, box, tm, dx_t, dy_t, *hflow) == want
    assert want[8:13] == (0, 0, 0, 0, 0)                                                   # rdt = 20
    assert D.psy.flow_courant_check(20.0, *flow, params=params) == r
    with pytest.raises(D.DlesmError, match="g and visc"):
        D.psy.flow_courant(20.0, *flow)
    big = FN.flow_courant(70.0, FC.G, FC.VISC, box, tm, dx_t, dy_t, *hflow)
    assert 0 < big.gravity_over < big.wet
    with pytest.raises(D.DlesmError, match=r"gravity_over: %d wet.*\(i, j\) = \(%d, %d\) on rank 1" % (
            big.gravity_over, *_at(g, big.gravity_index)[1:])):
        D.psy.flow_courant_check(70.0, *flow, params=params)
    with pytest.raises(D.DlesmError, match=r"advective_over: \d+ wet.*\(i, j\) = \(%d, %d\) on rank 1" % (
            _at(g, want.advective_index)[1:])):
        D.psy.flow_courant_check(20.0, *flow, params=params, advective_limit=1.0e-6)
    with pytest.raises(D.DlesmError, match=r"viscous_over: %d wet" % want.wet):
        D.psy.flow_courant_check(20.0, *flow, params=params, viscous_limit=1.0e-6)
    with pytest.raises(D.DlesmError, match=r"shallow: \d+ wet.*\(i, j\) = \(%d, %d\) on rank 1" % (
            _at(g, want.depth_index)[1:])):
        D.psy.flow_courant_check(20.0, *flow, params=params, depth_limit=10.5)
    ht = F["ht"]
    d = ht.get_data()
    wet = np.argwhere(tm[box[2] - 1:box[3], box[0] - 1:box[1]] > 0)[3]
    d[box[2] - 1 + wet[0], box[0] - 1 + wet[1]] = -20.0
    ht.set_data(d)
    with pytest.raises(D.DlesmError, match=r"invalid: 1 wet"):
        D.psy.flow_courant_check(20.0, *flow, params=params)
    # a stream of the caller's
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    assert D.psy.flow_courant(20.0, *flow, params=params, stream=s).invalid == 1
    # no wet cell: every location None, the estimate infinite
    g2 = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
    g2.decompose(nx, ny)
    it = g2.subdomain.internal
    D.grid_init(g2, 1000.0, 1000.0, tmask=np.zeros((it.ystop + 1, it.xstop + 1), dtype=np.int32))
    F2 = [D.r2d_field(g2, pt) for pt in (D.GO_U_POINTS, D.GO_V_POINTS, D.GO_T_POINTS, D.GO_T_POINTS)]
    for f in F2:
        f.set_data(np.ones((g2.ny, g2.nx)))
    r = D.psy.flow_courant(20.0, *F2, params=params)
    assert r == (0.0, 0.0, 0.0, math.inf, None, None, None, None, 0, 0, 0, 0, 0, 0, math.inf)
    assert D.psy.flow_courant_check(20.0, *F2, params=params) == r
    assert D.FlowCourant is D._cabi.FlowCourant
