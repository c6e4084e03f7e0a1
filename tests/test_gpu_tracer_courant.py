"""GPU tests (-m gpu) of the tracer schemes' Courant check, dlesm_tracer_courant_async_f64 / dlesm_tracer_courant_f64
(DESIGN.md section 6.14): every member of the record equals tests/tracer_courant_numpy.py, from the wave-tile kernel and from
the one-cell-per-thread kernel (HOOK key tracer_courant_kernel = 1), on the special-value and the plain case of tracer_cases at
its three shapes -- 260 x 12 spans three wave tiles of 63 chunks with both seams in the box, 131 x 10 is the odd pitch, 130 x 9
is swept on the sub-box (5, 100, 3, 8) -- at rdt = 600 and 3.0e6; with a base shifted by one element; on one-column and
one-row boxes, an empty box and an all-land box; on a tall box whose records need two levels of the reduction (the record
count is asserted on the host); on a wide row of eleven wave tiles.  What land holds changes no member.  A face number of
exactly face_limit counts, one an ulp below does not.  The asynchronous and the synchronous form, repeats and a second stream
agree.  Every refusal returns DLESM_EINVAL and leaves result_dev untouched.  The Python wrappers on a one-rank grid."""
import ctypes as C
import math

import numpy as np
import pytest

import tracer_cases as TC
import tracer_courant_cases as CC
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
    D._cabi.lib().dlesm_set_tuning(b"tracer_courant_kernel", value)


def _upload(tm, area_t, H, shift=0):
    import torch
    dev = _dev(torch, {"area_t": area_t, **{k: H[k] for k in CC.ARRAYS}}, shift)
    return torch.from_numpy(tm).cuda(), dev


def _args(rdt, ld, ny, box, tmd, dev, limits):
    return (float(rdt), ld, ny, *box, _p(tmd), _p(dev["area_t"]), *[_p(dev[n]) for n in CC.ARRAYS], float(limits[0]),
            float(limits[1]))


def _record(res):
    """the record in a device tensor of 8 doubles"""
    from dl_esm_inf_amd._cabi import TracerCourant
    return CN.Record(*TracerCourant.from_buffer_copy(res.cpu().numpy().tobytes()).as8())


def _device_call(D, rdt, ld, ny, box, tmd, dev, limits=CC.LIMITS, kernel=0, stream=None, sync=False):
    """one call; the asynchronous form into a sentinel-filled device record, or the synchronous one"""
    import torch
    L = D._cabi.lib()
    sp = None if stream is None else C.c_void_p(stream.cuda_stream)
    try:
        _hook(D, kernel)
        if sync:
            out = D._cabi.TracerCourant()
            rc = L.dlesm_tracer_courant_f64(*_args(rdt, ld, ny, box, tmd, dev, limits), C.byref(out), sp)
            assert rc == 0, L.dlesm_last_error()
            return CN.Record(*out.as8())
        res = torch.full((8,), SENTINEL, dtype=torch.float64, device="cuda")
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        rc = L.dlesm_tracer_courant_async_f64(*_args(rdt, ld, ny, box, tmd, dev, limits), _p(res), sp)
        assert rc == 0, L.dlesm_last_error()
        (stream or torch.cuda.current_stream()).synchronize()
    finally:
        _hook(D, 0)
    return _record(res)


def _run(D, tm, area_t, H, rdt, box, kernel=0, shift=0, limits=CC.LIMITS):
    """upload, call, and check that no input changed"""
    ny, ld = tm.shape
    tmd, dev = _upload(tm, area_t, H, shift)
    got = _device_call(D, rdt, ld, ny, box, tmd, dev, limits, kernel)
    for n in CC.ARRAYS:
        assert same(dev[n].cpu().numpy(), H[n]), n
    assert same(dev["area_t"].cpu().numpy(), area_t) and np.array_equal(tmd.cpu().numpy(), tm)
    return got


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("rdt", [TC.RDT, TC.RDT_BIG])
@pytest.mark.parametrize("kind", ["special", "plain"])
@pytest.mark.parametrize("ld,ny,box", TC.SPECIAL_SHAPES)
def test_every_member_equals_the_restatement(D, ld, ny, box, kind, rdt, kernel):
    tm, area_t, H = CC.host(kind, ld, ny, rdt)
    got = _run(D, tm, area_t, H, rdt, box, kernel)
    want = CC.reference(kind, ld, ny, box, rdt)
    print(got)
    assert CN.same_record(got, want), (got, want)


@pytest.mark.parametrize("kind,rdt", [("special", TC.RDT_BIG), ("plain", TC.RDT)])
@pytest.mark.parametrize("ld,ny,box", TC.SPECIAL_SHAPES)
def test_shifted_base(D, ld, ny, box, kind, rdt):
    """every double array 8 bytes off a 16-byte boundary: the one-cell-per-thread kernel without the key"""
    tm, area_t, H = CC.host(kind, ld, ny, rdt)
    got = _run(D, tm, area_t, H, rdt, box, 0, shift=1)
    assert CN.same_record(got, CC.reference(kind, ld, ny, box, rdt)), got


SMALL = [(2, 259, 5, 5), (2, 259, 2, 2), (2, 259, 11, 11),                   # one row: middle, first, last
         (127, 127, 2, 11), (126, 126, 2, 11), (2, 2, 2, 11), (259, 259, 2, 11),   # one column: beside the seam, the edges
         (21, 21, 5, 5)]                                                     # one cell


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("box", SMALL)
def test_one_row_and_one_column_boxes(D, box, kernel):
    rdt = TC.RDT_BIG
    tm, area_t, H = CC.host("special", 260, 12, rdt)
    got = _run(D, tm, area_t, H, rdt, box, kernel)
    assert CN.same_record(got, CC.reference("special", 260, 12, box, rdt)), got


@pytest.mark.parametrize("kernel", [0, 1])
def test_empty_and_all_land_boxes(D, kernel):
    """{0, 0, -1, -1, 0, 0, 0, 0}; the empty box reads nothing (its arrays' pointers are only checked)"""
    tm, area_t, H = CC.plain_host(130, 9)
    for box in [(9, 8, 2, 5), (2, 129, 5, 4)]:
        assert _run(D, tm, area_t, H, TC.RDT, box, kernel) == CN.EMPTY
    for value in (0, -1):
        assert _run(D, np.full_like(tm, value), area_t, H, TC.RDT, (2, 129, 2, 8), kernel) == CN.EMPTY


def _records(ld, box, kernel):
    """records the sweep leaves = its workgroups, for a box one wave tile wide: the tile form packs four waves, one per row,
    into a workgroup; the one-cell-per-thread form has 256 columns and at most 4096
    row strides"""
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
    """66 x 4200 (test_gpu_tracer_hancock.py's TALL): 1050 records from the tile form, 4096 from the one-cell-per-thread form
    (whose row loop makes its second trip) -- more than one workgroup of a level holds, so a second level runs; fewer than
    1024**2, beyond which a third would"""
    ld, ny = 66, 4200
    box = (2, ld - 1, 2, ny - 1)
    n = _records(ld, box, kernel)
    assert n == (1050 if kernel == 0 else 4096) and LEVEL_CHUNK < n <= LEVEL_CHUNK ** 2
    tm, area_t, H = CC.plain_host(ld, ny)
    want = CC.reference("plain", ld, ny, box, TC.RDT_BIG)
    got = _run(D, tm, area_t, H, TC.RDT_BIG, box, kernel)
    assert CN.same_record(got, want), (got, want)
    assert want.face_index // ld > 0 and want.wet > 100000 and want.face_over > 0


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("box", [(2, 1299, 2, 7), (301, 1291, 3, 6)])
def test_wide_row(D, box, kernel):
    """1300 x 8: eleven wave tiles a row (padded with idle ones by the launcher's block shape), every seam in the box; and a
    box that starts mid-row"""
    tm, area_t, H = CC.plain_host(1300, 8)
    want = CC.reference("plain", 1300, 8, box, TC.RDT_BIG)
    got = _run(D, tm, area_t, H, TC.RDT_BIG, box, kernel)
    assert CN.same_record(got, want), (got, want)


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("kind,rdt", [("special", TC.RDT_BIG), ("plain", TC.RDT_BIG)])
@pytest.mark.parametrize("ld,ny,box", TC.SPECIAL_SHAPES)
def test_land_changes_no_member(D, ld, ny, box, kind, rdt, kernel):
    """NaN in un / vn on every face that touches land and in area_t, ht, sshn_t on every land cell"""
    tm, area_t, H = CC.host(kind, ld, ny, rdt)
    a2, H2 = CC.land_overwritten(tm, area_t, H)
    got = _run(D, tm, a2, H2, rdt, box, kernel)
    assert CN.same_record(got, CC.reference(kind, ld, ny, box, rdt)), got


@pytest.mark.parametrize("kernel", [0, 1])
def test_a_face_at_the_limit_counts(D, kernel):
    rdt, (ld, ny, box) = TC.RDT, TC.SPECIAL_SHAPES[0]
    tm, area_t, H = CC.special_host(ld, ny, rdt)
    one = (CC.PROBE[0], CC.PROBE[0], CC.PROBE[1], CC.PROBE[1])
    for top, over in ((1.0, 1), (-1.0, 1), (TC.ONE_BELOW, 0)):
        H2 = CC.patch_probe(H, top)
        r = _run(D, tm, area_t, H2, rdt, one, kernel, limits=(1.0, 1.0))
        assert r.face_max == abs(top) and r.face_over == over and r.wet == 1 and r.invalid == 0, r
        whole = _run(D, tm, area_t, H2, rdt, box, kernel, limits=(1.0, 1.0))
        assert CN.same_record(whole, CN.tracer_courant(rdt, box, tm, area_t, *CC.flow(H2), 1.0, 1.0)), whole


def test_forms_repeats_and_streams_agree(D):
    import torch
    rdt, (ld, ny, box) = TC.RDT_BIG, TC.SPECIAL_SHAPES[0]
    tm, area_t, H = CC.host("special", ld, ny, rdt)
    want = CC.reference("special", ld, ny, box, rdt)
    tmd, dev = _upload(tm, area_t, H)
    second = torch.cuda.Stream()
    for kernel in (0, 1):
        got = [_device_call(D, rdt, ld, ny, box, tmd, dev, kernel=kernel) for _ in range(3)]
        got.append(_device_call(D, rdt, ld, ny, box, tmd, dev, kernel=kernel, sync=True))
        got.append(_device_call(D, rdt, ld, ny, box, tmd, dev, kernel=kernel, stream=second))
        got.append(_device_call(D, rdt, ld, ny, box, tmd, dev, kernel=kernel, stream=second, sync=True))
        for g in got:
            assert CN.same_record(g, want), (kernel, g, want)


def test_refusals(D):
    """DLESM_EINVAL before anything is launched; result_dev keeps its bits"""
    import torch
    L = D._cabi.lib()
    ld, ny, box = 130, 9, (2, 129, 2, 8)
    tm, area_t, H = CC.plain_host(ld, ny)
    tmd, dev = _upload(tm, area_t, H)
    res = torch.full((8,), SENTINEL, dtype=torch.float64, device="cuda")
    good = list(_args(TC.RDT, ld, ny, box, tmd, dev, CC.LIMITS))

    def refused(args, result=None, stream=None):
        result = _p(res) if result is None else result
        rc = L.dlesm_tracer_courant_async_f64(*args, result, stream)
        host = D._cabi.TracerCourant(1.0, 2.0, 3, 4, 5, 6, 7, 8)
        rc2 = L.dlesm_tracer_courant_f64(*args, C.byref(host), stream)
        torch.cuda.synchronize()
        return (rc == EINVAL and rc2 == EINVAL and (res == SENTINEL).all().item()
                and host.as8() == (1.0, 2.0, 3, 4, 5, 6, 7, 8))

    assert L.dlesm_tracer_courant_async_f64(*good, _p(res), None) == 0
    torch.cuda.synchronize()
    assert (res != SENTINEL).all().item()
    res.fill_(SENTINEL)
    for k in range(7, 17):                                                     # a null pointer: tmask .. sshn_v
        bad = list(good)
        bad[k] = None
        assert refused(bad), k
    assert L.dlesm_tracer_courant_async_f64(*good, None, None) == EINVAL
    assert L.dlesm_tracer_courant_f64(*good, None, None) == EINVAL
    for k in range(8, 17):                                                     # a double array 4 bytes off
        bad = list(good)
        bad[k] = C.c_void_p(good[k].value + 4)
        assert refused(bad), k
    bad = list(good)
    bad[7] = C.c_void_p(good[7].value + 2)                                     # the mask 2 bytes off
    assert refused(bad)
    for b in [(1, 129, 2, 8), (2, 130, 2, 8), (2, 129, 1, 8), (2, 129, 2, 9), (0, 5, 2, 8), (2, 131, 2, 8)]:
        bad = list(good)                                                       # a box without its ring
        bad[3:7] = b
        assert refused(bad), b
    for lim in (math.nan, 0.0, -0.0, -1.0, -math.inf):
        for k in (17, 18):
            bad = list(good)
            bad[k] = lim
            assert refused(bad), (k, lim)
    for name in ("area_t",) + CC.ARRAYS:                                       # result_dev inside an input array
        t = dev[name]
        rc = L.dlesm_tracer_courant_async_f64(*good, C.c_void_p(t.data_ptr() + 8 * (ld * ny - 8)), None)
        torch.cuda.synchronize()
        assert rc == EINVAL and same(t.cpu().numpy(), area_t if name == "area_t" else H[name]), name
    rc = L.dlesm_tracer_courant_async_f64(*good, C.c_void_p(tmd.data_ptr() + 4 * (ld * ny - 16)), None)
    assert rc == EINVAL and np.array_equal(tmd.cpu().numpy(), tm)
    # under stream capture the call is refused before it enqueues anything: the capture stays intact and replays
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    x = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        x.add_(1.0)
        rc = L.dlesm_tracer_courant_async_f64(*good, _p(res), sp)
        host = D._cabi.TracerCourant(1.0, 2.0, 3, 4, 5, 6, 7, 8)
        rc2 = L.dlesm_tracer_courant_f64(*good, C.byref(host), sp)
    assert rc == EINVAL and rc2 == EINVAL and host.as8() == (1.0, 2.0, 3, 4, 5, 6, 7, 8)
    graph.replay()
    torch.cuda.synchronize()
    assert (x == 1.0).all().item() and (res == SENTINEL).all().item()
    # and the arguments that were refused above still work
    assert L.dlesm_tracer_courant_async_f64(*good, _p(res), None) == 0
    torch.cuda.synchronize()
    assert CN.same_record(_record(res), CC.reference("plain", ld, ny, box, TC.RDT))


def _points(D):
    T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
    return (U, V, T, U, V, T, U, V)


def _grid_case(D, nx, ny, alignment):
    """a one-rank grid with a -1/0/1 user mask and hashed flow fields (test_gpu_fortran_tracer_hancock.py's inputs)"""
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
    F, H = {}, {}
    names = ("un", "vn", "ht", "hu", "hv", "sshn_t", "sshn_u", "sshn_v")                 # the wrapper's order
    for k, (name, pt) in enumerate(zip(names, _points(D)), start=2):
        f = D.r2d_field(g, pt)
        D.psy.hash_init(f, 500 + k)
        d = f.get_data()
        d = 0.4 * d - 0.2 if k in (2, 3) else 10.0 + d if k in (4, 5, 6) else 0.05 * d
        f.set_data(d)
        F[name], H[name] = f, np.ascontiguousarray(d)
    return g, [F[n] for n in names], H


@pytest.mark.parametrize("nx,ny,alignment", [(257, 6, 2), (128, 4, 1)])
def test_python_wrappers(D, nx, ny, alignment):
    """psy.tracer_courant on arrays (260, 9) and (131, 7): the restatement's record, locations as (rank, i, j), the estimate
    of rdt; psy.tracer_courant_check raises on each of the three counts and returns the result otherwise"""
    g, F, H = _grid_case(D, nx, ny, alignment)
    tm, area_t = g.tmask_device.cpu().numpy(), g.area_t_device.cpu().numpy()
    box = F[5].internal.box()
    for rdt in (1.0e7, 100.0):
        want = CN.tracer_courant(rdt, box, tm, area_t, *CC.flow(H))
        r = D.psy.tracer_courant(rdt, *F)
        print(r)
        assert (r.face_max, r.outflow_max) == (want.face_max, want.outflow_max)
        assert (r.face_over, r.outflow_over, r.invalid, r.wet) == tuple(want[4:])
        assert r.face_at == (1, want.face_index % g.nx + 1, want.face_index // g.nx + 1)
        assert r.outflow_at == (1, want.outflow_index % g.nx + 1, want.outflow_index // g.nx + 1)
        assert r.rdt_limit == CN.rdt_limit(rdt, want) and 0.0 < r.rdt_limit < math.inf
    assert want.face_over == 0 and want.outflow_over == 0 and want.invalid == 0          # rdt = 100
    assert D.psy.tracer_courant_check(100.0, *F) == r
    big = CN.tracer_courant(1.0e7, box, tm, area_t, *CC.flow(H))
    assert big.face_over > 0 and big.outflow_over > 0 and big.face_over < big.wet
    with pytest.raises(D.DlesmError, match=r"face_over: %d wet.*\(i, j\) = \(%d, %d\) on rank 1" % (
            big.face_over, big.face_index % g.nx + 1, big.face_index // g.nx + 1)):
        D.psy.tracer_courant_check(1.0e7, *F)
    with pytest.raises(D.DlesmError, match=r"outflow_over: %d wet.*\(i, j\) = \(%d, %d\) on rank 1" % (
            big.outflow_over, big.outflow_index % g.nx + 1, big.outflow_index // g.nx + 1)):
        D.psy.tracer_courant_check(1.0e7, *F, face_limit=1.0e30)
    assert D.psy.tracer_courant_check(1.0e7, *F, face_limit=1.0e30, outflow_limit=1.0e30).face_over == 0
    ht = F[2]
    d = ht.get_data()
    wet = np.argwhere(tm[box[2] - 1:box[3], box[0] - 1:box[1]] > 0)[3]
    d[box[2] - 1 + wet[0], box[0] - 1 + wet[1]] = np.nan
    ht.set_data(d)
    with pytest.raises(D.DlesmError, match=r"invalid: \d+ wet"):
        D.psy.tracer_courant_check(100.0, *F)
    # a stream of the caller's
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    assert D.psy.tracer_courant(100.0, *F, stream=s).invalid >= 1
    # no wet cell: both locations None, the estimate infinite
    g2 = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
    g2.decompose(nx, ny)
    it = g2.subdomain.internal
    D.grid_init(g2, 1000.0, 1000.0, tmask=np.zeros((it.ystop + 1, it.xstop + 1), dtype=np.int32))
    F2 = [D.r2d_field(g2, pt) for pt in _points(D)]
    for f in F2:
        f.set_data(np.ones((g2.ny, g2.nx)))
    r = D.psy.tracer_courant(100.0, *F2)
    assert r == (0.0, 0.0, None, None, 0, 0, 0, 0, math.inf)
    assert D.psy.tracer_courant_check(100.0, *F2) == r
    assert D.TracerCourant is D._cabi.TracerCourant
