"""GPU tests (-m gpu) of tracer transport, dlesm_tracer_step_f64: bit for bit tests/tracer_numpy.py on
whole arrays -- box, ring and padding of sentinel-filled outputs -- with the wave tile and the general path (HOOK key
tracer_kernel, odd pitches, unaligned bases), for 1..8 tracers of different data, on sub-boxes, on masks of all land, all wet,
a wet stripe and open edges; boxes of 4200 rows, which make the second trip of the one-cell-per-thread kernel's row loop
(gridDim.y = 4096); land invariance on the device; the refusals, which write nothing; a time loop with the step
captured into a hipGraph; six open-channel steps through the Python wrappers against the CPU loop; one 4096^2 case.

No case past 2^31 cells.  One written after tests/test_gpu_nemolite_large_index.py (shared read-only inputs, 112 GB of arrays,
row bands swept again as small arrays) could not be run on a GPU while this file was written, so whether it fits the few
seconds a test here may take is not known, and it is left out.  The kernels index with size_t row offsets, as the kernels that
test covers do."""
import ctypes as C
import os

import numpy as np
import pytest

import open_bc_numpy as B
import tracer_cases as TC
import tracer_numpy as TN
from nemolite_boxes import INS, METRICS, OUTS, _dev

pytestmark = pytest.mark.gpu

SHAPES = [(300, 70), (301, 41), (256, 33), (1000, 37), (130, 20), (4100, 9), (6, 5)]


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
    return None if t is None else C.c_void_p(t.data_ptr())


def _ptrs(ts):
    return (C.c_void_p * max(len(ts), 1))(*[None if t is None else t.data_ptr() for t in ts])


def _call(D, rdt, ld, ny, box, tmd, area, I, ci, co, k=None, stream=None):
    """dlesm_tracer_step_f64 on device tensors; returns its code"""
    return D._cabi.lib().dlesm_tracer_step_f64(rdt, ld, ny, *box, _p(tmd), _p(area), *[_p(I[n]) for n in TC.FLOW], _ptrs(ci),
                                               _ptrs(co), len(ci) if k is None else k, stream)


def _case(torch, ld, ny, k, seed, tm=None, shift=0):
    rng = np.random.default_rng(seed)
    if tm is None:
        tm = TC.random_mask(rng, ny, ld)
    area_t, H = TC.flow_inputs(rng, tm)
    c_in, c_out = TC.tracers(rng, tm.shape, k)
    dev = _dev(torch, {"area_t": area_t, **H}, shift)
    ci = list(_dev(torch, {str(n): a for n, a in enumerate(c_in)}, shift).values())
    co = list(_dev(torch, {str(n): a for n, a in enumerate(c_out)}, shift).values())
    return tm, area_t, H, c_in, c_out, torch.from_numpy(tm).cuda(), dev, ci, co


def _check(D, ld, ny, box, k, kernel, seed, tm=None, shift=0):
    """one call against tracer_numpy in every cell of every output; the inputs keep their bits; returns (tm, outputs)"""
    import torch
    tm, area_t, H, c_in, c_out, tmd, dev, ci, co = _case(torch, ld, ny, k, seed, tm, shift)
    want = TC.reference(TC.RDT, box, tm, area_t, H, c_in, c_out)
    try:
        _set_tuning(D, tracer_kernel=kernel)
        rc = _call(D, TC.RDT, ld, ny, box, tmd, dev["area_t"], dev, ci, co)
        assert rc == 0, D._cabi.lib().dlesm_last_error()
        torch.cuda.synchronize()
    finally:
        _set_tuning(D, tracer_kernel=0)
    got = [t.cpu().numpy() for t in co]
    for n in range(k):
        assert TN.same(got[n], want[n]), (n, int((got[n] != want[n]).sum()))
        assert TN.same(ci[n].cpu().numpy(), c_in[n]), n
    for n in TC.FLOW:
        assert TN.same(dev[n].cpu().numpy(), H[n]), n
    assert np.array_equal(tmd.cpu().numpy(), tm)
    return tm, got


@pytest.mark.parametrize("ld,ny", SHAPES)
@pytest.mark.parametrize("kernel", [0, 1])
def test_shapes_and_paths(D, ld, ny, kernel):
    """odd and even pitches, several wave tiles per row, a tile that ends mid-row, the smallest array with a ring; random
    -1/0/1 masks, non-uniform metrics, two tracers.  kernel = 1: the HOOK key forces the general path"""
    tm, got = _check(D, ld, ny, (2, ld - 1, 2, ny - 1), 2, kernel, ld * 7 + ny)
    if ld > 8:
        assert (got[0] != TC.SENTINEL).any() and (got[0][1:-1, 1:-1] == TC.SENTINEL).any()


# 4200 rows: the second trip of the one-cell-per-thread kernel's row loop (kernel = 1; 13 is an odd pitch, which takes that
# kernel with kernel = 0), and the tile at the same height
@pytest.mark.parametrize("ld,ny,kernel", [(12, 4200, 1), (13, 4200, 0), (66, 4200, 0)])
def test_tall_boxes(D, ld, ny, kernel):
    """two tracers against the array restatement; wet cells were written beyond row 4096 of the box"""
    tm, got = _check(D, ld, ny, (2, ld - 1, 2, ny - 1), 2, kernel, ld * 7 + ny)
    far = tm[4097:ny - 1, 1:ld - 1] > 0              # the box starts at row 1 (0-based): its rows 4096 ..
    assert far.sum() > ld and all((g[4097:ny - 1, 1:ld - 1][far] != TC.SENTINEL).all() for g in got)


@pytest.mark.parametrize("ld,ny", [(300, 70), (4100, 9)])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("kernel", [0, 1])
def test_tracer_counts(D, ld, ny, k, kernel):
    """every instantiation (1..4 tracers a launch) and the two-launch calls (5, 8); the tracers hold different data, so a
    swapped pointer shows"""
    _check(D, ld, ny, (2, ld - 1, 2, ny - 1), k, kernel, 1000 + ld + k)


@pytest.mark.parametrize("ld,ny,box,shift", [
    (300, 70, (37, 250, 5, 60), 0),          # a box away from the origin
    (300, 70, (64, 66, 2, 19), 0),           # a three-column box
    (130, 20, (64, 66, 2, 19), 0),
    (300, 70, (2, 129, 10, 10), 0),          # a one-row box
    (130, 20, (2, 129, 10, 10), 0),
    (300, 70, (2, 299, 2, 69), 1),           # bases 8 bytes off a 16-byte boundary
    (130, 20, (2, 129, 2, 19), 1),
    (300, 70, (37, 250, 5, 60), 1),
])
@pytest.mark.parametrize("kernel", [0, 1])
def test_sub_boxes_and_bases(D, ld, ny, box, shift, kernel):
    _check(D, ld, ny, box, 3, kernel, ld + 5 * ny + 11 * shift + box[0])


@pytest.mark.parametrize("ld,ny", [(300, 70), (130, 20)])
@pytest.mark.parametrize("kernel", [0, 1])
def test_an_empty_box_writes_nothing(D, ld, ny, kernel):
    tm, got = _check(D, ld, ny, (5, 4, 2, ny - 1), 2, kernel, 3)
    assert all((g == TC.SENTINEL).all() for g in got)
    tm, got = _check(D, ld, ny, (2, ld - 1, 9, 8), 2, kernel, 4)
    assert all((g == TC.SENTINEL).all() for g in got)


def _masks(ld, ny):
    land = np.zeros((ny, ld), dtype=np.int32)
    wet = np.ones((ny, ld), dtype=np.int32)
    row = land.copy()
    row[ny // 2, :] = 1                                            # a wet stripe one cell wide along x ...
    col = land.copy()
    col[:, 131] = 1                                                # ... and along y, in the second wave tile
    opn = wet.copy()
    opn[:, 0] = opn[0, :] = 0
    opn[:, 1] = opn[1, :] = -1                                     # open west and south edges of the box
    opn[-3:, :] = 0
    return {"land": land, "wet": wet, "row": row, "col": col, "open": opn}


@pytest.mark.parametrize("which", ["land", "wet", "row", "col", "open"])
@pytest.mark.parametrize("kernel", [0, 1])
def test_masks(D, which, kernel):
    """all land: nothing written; all wet; a wet stripe one cell wide; open west and south edges (the velocities are random:
    inflow and outflow through the open faces)"""
    ld, ny = 300, 70
    tm = _masks(ld, ny)[which]
    box = (2, ld - 1, 2, ny - 1)
    _, got = _check(D, ld, ny, box, 2, kernel, 77, tm=tm)
    written = got[0] != TC.SENTINEL
    inside = np.zeros_like(written)
    inside[1:-1, 1:-1] = True
    assert np.array_equal(written, inside & (tm > 0))
    if which == "land":
        assert not written.any()
    if which == "open":
        assert written[2, 2:-1].all() and written[2:-3, 2].all() and not written[1, :].any() and not written[:, 1].any()


@pytest.mark.parametrize("fill", TC.LAND_FILLS)
@pytest.mark.parametrize("kernel", [0, 1])
def test_land_invariance_on_the_device(D, fill, kernel):
    """six steps; before each, every tracer's land cells hold `fill` and un / vn NaN on every face that touches land: every
    wet cell equals the CPU run without the overwrites, bit for bit"""
    import torch
    ld, ny, k = 300, 41, 2
    box = (2, ld - 1, 2, ny - 1)
    rng = np.random.default_rng(7)
    tm = TC.random_mask(rng, ny, ld)
    area_t, H = TC.flow_inputs(rng, tm)
    c0, _ = TC.tracers(rng, tm.shape, k)
    clean = ([c.copy() for c in c0], [c.copy() for c in c0])
    H2, _ = TC.overwrite_land(tm, H, [], fill)
    assert np.isnan(H2["un"]).sum() > 100 and np.isnan(H2["vn"]).sum() > 100
    dev = _dev(torch, {"area_t": area_t, **H2}, 0)
    tmd = torch.from_numpy(tm).cuda()
    land = torch.from_numpy(tm == 0).cuda()
    a = [torch.from_numpy(c).cuda() for c in c0]
    b = [torch.from_numpy(c).cuda() for c in c0]
    wet = tm > 0
    try:
        _set_tuning(D, tracer_kernel=kernel)
        for step in range(6):
            TN.tracer_step(TC.RDT, box, tm, area_t, *[H[n] for n in TC.FLOW], clean[0], clean[1])
            for t in a:
                t[land] = fill
            assert _call(D, TC.RDT, ld, ny, box, tmd, dev["area_t"], dev, a, b) == 0, D._cabi.lib().dlesm_last_error()
            torch.cuda.synchronize()
            for n in range(k):
                assert TN.same(b[n].cpu().numpy()[wet], clean[1][n][wet]), (step, n)
            clean = (clean[1], clean[0])
            a, b = b, a
    finally:
        _set_tuning(D, tracer_kernel=0)


def test_refusals_write_nothing(D):
    """0 and 9 tracers, c_out[0] == c_in[0], c_out[1] == c_out[0], c_out[0] == ssha, an output over tmask, a box without its
    ring, null pointers: DLESM_EINVAL before anything is launched"""
    import torch
    L = D._cabi.lib()
    ld, ny = 64, 20
    box = (2, ld - 1, 2, ny - 1)
    tmd = torch.ones((ny, ld), dtype=torch.int32, device="cuda")
    I = {n: torch.full((ny, ld), 1.0, dtype=torch.float64, device="cuda") for n in TC.FLOW + ("area_t",)}
    ci = [torch.full((ny, ld), 2.0, dtype=torch.float64, device="cuda") for _ in range(9)]
    co = [torch.full((ny, ld), -7.0, dtype=torch.float64, device="cuda") for _ in range(9)]
    big = torch.full((2 * ny, ld), -7.0, dtype=torch.float64, device="cuda")
    half = big[ny // 2:ny // 2 + ny]

    def call(box=box, tmd=tmd, I=I, ci=ci[:2], co=co[:2], k=None, area="area_t"):
        return _call(D, 20.0, ld, ny, box, tmd, I[area] if area else None, I, ci, co, k)

    assert call() == 0
    torch.cuda.synchronize()
    for t in co[:2]:
        t.fill_(-7.0)
    cases = {
        "k=0": call(ci=[], co=[], k=0), "k=9": call(ci=ci, co=co, k=9), "k=-1": call(k=-1),
        "out is in": call(co=[ci[0], co[1]]), "out is the other in": call(co=[ci[1], co[1]]),
        "out twice": call(co=[co[0], co[0]]), "outs overlap": call(co=[big, half]),
        "out is ssha": call(co=[I["ssha"], co[1]]), "out is un": call(co=[co[0], I["un"]]),
        "out is area_t": call(co=[I["area_t"], co[1]]), "out over tmask": call(co=[tmd, co[1]]),
        "no west ring": call(box=(1, ld - 1, 2, ny - 1)), "no east ring": call(box=(2, ld, 2, ny - 1)),
        "no south ring": call(box=(2, ld - 1, 1, ny - 1)), "no north ring": call(box=(2, ld - 1, 2, ny)),
        "null tmask": call(tmd=None), "null area_t": call(area=None), "null vn": call(I={**I, "vn": None}),
        "null ssha": call(I={**I, "ssha": None}), "null c_in[1]": call(ci=[ci[0], None]),
        "null c_out[0]": call(co=[None, co[1]]),
        "null arrays": L.dlesm_tracer_step_f64(20.0, ld, ny, *box, _p(tmd), _p(I["area_t"]), *[_p(I[n]) for n in TC.FLOW], None,
                                               None, 1, None),
    }
    assert all(rc == D._cabi.EINVAL for rc in cases.values()), cases
    torch.cuda.synchronize()
    assert bool((big == -7.0).all()) and all(bool((t == -7.0).all()) for t in co)
    assert all(bool((t == 2.0).all()) for t in ci) and all(bool((t == 1.0).all()) for t in I.values())
    assert bool((tmd == 1).all())


# ---- through the Python wrappers ------------------------------------------------------------------------------------
def _grid(D, nx, ny, user, dxy, ndomains=None, alignment=64):
    os.environ["DL_ESM_ALIGNMENT"] = str(alignment)
    try:
        g = D.grid_type(D.GO_ARAKAWA_C, (1, 1, 2), D.GO_OFFSET_NE)
        if ndomains is None:
            g.decompose(nx, ny)
        else:
            g.decompose(nx, ny, ndomains=ndomains)
        D.grid_init(g, dxy, dxy, tmask=user)
    finally:
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


def _tfields(D, g, arrays):
    import torch
    out = []
    for a in arrays:
        f = D.r2d_field(g, D.GO_T_POINTS)
        f.data.copy_(torch.from_numpy(a))
        out.append(f)
    return out


def _host_grid(D, g):
    import momentum_numpy as M
    return M.SimpleNamespace(tmask=g.tmask_device.cpu().numpy(), **{k: getattr(g, k + "_device").cpu().numpy() for k in METRICS},
                             fcor_u=g.fcor[2].cpu().numpy(), fcor_v=g.fcor[3].cpu().numpy())


def _tracer_order(F):
    return [F[k] for k in ("ssha", "un", "vn", "ht", "hu", "hv", "sshn_t", "sshn_u", "sshn_v")]


@pytest.mark.parametrize("nx,alignment", [(200, 64), (198, 1)])
def test_open_channel_time_loop(D, nx, alignment):
    """nx x 40, open first and last internal columns, a current along the channel and a tide: six steps of
    invoke_nemolite_step + invoke_tracer_step with three tracers, every array bit for bit against the CPU loop after every
    step.  DL_ESM_ALIGNMENT 64: the tile; 1: an odd pitch, the general path"""
    import torch
    ny = 40
    g = _grid(D, nx, ny, TC.channel_user_mask(nx, ny), TC.CHANNEL_DXY, alignment=alignment)
    assert (g.nx % 2 == 0) == (alignment == 64)
    D.psy.coriolis(g)
    G = _host_grid(D, g)
    H = TC.channel_state(G.tmask, nx, ny)
    F = _fields(D, g, H)
    box = F["ssha"].internal.box()
    c_in, c_out = TC.channel_tracers(G.tmask)
    third = np.where(G.tmask != 0, 5.0 + np.random.default_rng(5).random(G.tmask.shape), 3.0)
    c_in.append(third.copy())
    c_out.append(third.copy())
    Ci, Co = _tfields(D, g, c_in), _tfields(D, g, c_out)
    prm = D.psy.momentum_params(*TC.CHANNEL_PRM)
    rdt = TC.CHANNEL_PRM[0]
    for step in range(6):
        ssh_bc = D.psy.tide_ssh(*TC.CHANNEL_TIDE, (step + 1) * rdt)
        D.psy.invoke_nemolite_step(prm, *[F[k] for k in OUTS], *[F[k] for k in INS], ssh_bc=ssh_bc)
        D.psy.invoke_tracer_step(rdt, Co, Ci, *_tracer_order(F))
        TC.cpu_step(G, box, H, B.tide(*TC.CHANNEL_TIDE, (step + 1) * rdt), c_in, c_out, TC.CHANNEL_PRM)
        torch.cuda.synchronize()
        for k in TC.STATE:
            assert TN.same(F[k].get_data(), H[k]), (step, k)
        for n in range(3):
            assert TN.same(Co[n].get_data(), c_out[n]), (step, n)
        for a, b in TC.ROTATE:
            F[a], F[b] = F[b], F[a]
        TC.rotate(H)
        Ci, Co, c_in, c_out = Co, Ci, c_out, c_in
    wet = G.tmask > 0
    assert np.abs(c_in[0][wet] - 1.0).max() <= 6 * 32 * 2.0 ** -52
    assert np.ptp(c_in[1][wet]) > 0.5 and all(np.isfinite(c[wet]).all() for c in c_in)


def test_time_loop_captured_into_a_graph(D):
    """a closed basin, ten steps of invoke_nemolite_step + invoke_tracer_step with pointer rotation captured into ONE hipGraph
    and replayed once: every array equals the uncaptured loop"""
    import torch
    nx, ny = 254, 60
    user = np.ones((ny + 2, nx + 2), dtype=np.int32)
    user[0, :] = user[-1, :] = 0
    user[:, 0] = user[:, -1] = 0
    user[20:30, 100:140] = 0
    g = _grid(D, nx, ny, user, TC.CHANNEL_DXY)
    D.psy.coriolis(g)
    tm = g.tmask_device.cpu().numpy()
    H = TC.channel_state(tm, nx, ny, current=0.0)
    c0, _ = TC.channel_tracers(tm)
    prm = D.psy.momentum_params(*TC.CHANNEL_PRM)
    rdt = TC.CHANNEL_PRM[0]

    def loop(F, Ci, Co, stream):
        for _ in range(10):
            D.psy.invoke_nemolite_step(prm, *[F[k] for k in OUTS], *[F[k] for k in INS], stream=stream)
            D.psy.invoke_tracer_step(rdt, Co, Ci, *_tracer_order(F), stream=stream)
            for a, b in TC.ROTATE:
                F[a], F[b] = F[b], F[a]
            Ci, Co = Co, Ci
        return Ci

    F1, A1, B1 = _fields(D, g, H), _tfields(D, g, c0), _tfields(D, g, c0)
    last1 = loop(dict(F1), A1, B1, None)
    torch.cuda.synchronize()
    F2, A2, B2 = _fields(D, g, H), _tfields(D, g, c0), _tfields(D, g, c0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        last2 = loop(dict(F2), A2, B2, s)
    torch.cuda.synchronize()
    assert TN.same(A2[1].get_data(), c0[1]) and TN.same(B2[1].get_data(), c0[1])      # captured, not run
    with torch.cuda.stream(s):
        graph.replay()
    torch.cuda.synchronize()
    for k in TC.STATE:
        assert TN.same(F2[k].get_data(), F1[k].get_data()), k
    for n in range(2):
        assert TN.same(A2[n].get_data(), A1[n].get_data()) and TN.same(B2[n].get_data(), B1[n].get_data()), n
    assert last1 is A1 and last2 is A2                             # an even number of steps: the pointers are back
    wet = tm > 0
    dye = A1[1].get_data()
    assert np.isfinite(dye[wet]).all() and not TN.same(dye, c0[1])
    assert np.abs(A1[0].get_data()[wet] - 1.0).max() <= 10 * 32 * 2.0 ** -52
    del graph


def test_python_wrapper_refusals(D):
    """a decomposed grid: invoke_tracer_step stops and names invoke_tracer_step_dm; lists of different length, no tracer and
    nine tracers are refused; nothing is written"""
    import torch
    nx, ny = 64, 32
    gd = _grid(D, nx, ny, None, 1000.0, ndomains=2)
    assert gd.decomp.ndomains == 2
    shape = (gd.ny, gd.nx)
    H = {k: np.full(shape, 1.0) for k in TC.STATE}
    F = _fields(D, gd, H)
    Ci, Co = _tfields(D, gd, [np.full(shape, 2.0)] * 2), _tfields(D, gd, [np.full(shape, -7.0)] * 2)
    with pytest.raises(D._cabi.GoceanStop, match="invoke_tracer_step_dm"):
        D.psy.invoke_tracer_step(20.0, Co, Ci, *_tracer_order(F))
    g = _grid(D, nx, ny, np.ones((ny + 2, nx + 2), dtype=np.int32), 1000.0)
    F1 = _fields(D, g, {k: np.full((g.ny, g.nx), 1.0) for k in TC.STATE})
    Ci1 = _tfields(D, g, [np.full((g.ny, g.nx), 2.0)] * 9)
    Co1 = _tfields(D, g, [np.full((g.ny, g.nx), -7.0)] * 9)
    with pytest.raises(D._cabi.DlesmError):
        D.psy.invoke_tracer_step(20.0, Co1[:1], Ci1[:2], *_tracer_order(F1))
    with pytest.raises(D._cabi.DlesmError):
        D.psy.invoke_tracer_step(20.0, [], [], *_tracer_order(F1))
    with pytest.raises(D._cabi.DlesmError):
        D.psy.invoke_tracer_step(20.0, Co1, Ci1, *_tracer_order(F1))
    torch.cuda.synchronize()
    assert all((f.get_data() == -7.0).all() for f in Co + Co1)


def test_4096_whole_fields(D):
    """one sweep at 4096^2 with four tracers (the tile), whole fields"""
    n = 4096
    _check(D, n + 2, n + 2, (2, n + 1, 2, n + 1), 4, 0, 4096)
