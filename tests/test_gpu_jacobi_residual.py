"""GPU test (-m gpu): the Jacobi step with its residual, dlesm_stencil5_resid_f64.
- `out` is bit for bit what dlesm_stencil5_f64 writes, on whole sentinel-filled arrays: even and odd pitches, box starts at
  every column mod 16, one-row / one-column / one-cell boxes, a base 8 bytes off 16 (8-byte lanes);
- max|out - in| is exact (random data, IEEE specials, a NaN gives NaN);
- SUM (out - in)^2 keeps its bits over repeats, streams, launch shapes, padding, tile heights and the planning call, and is within
  1e-12 of math.fsum;
- an empty box writes 0.0, every refusal leaves `out` and the result alone;
- the headline size against torch, a box of more than 2^31 elements against a chunked device max;
- a Laplace solve to max <= 1e-9 through psy.invoke_jacobi5_residual: the step count and the final field of the oracle's loop."""
import ctypes as C
import math

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
MAX, SUMSQ = 0, 1
SENT = -7.25


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    import dl_esm_inf_amd as d
    torch.cuda.set_device(0)
    d.parallel_init(0, 1)
    return torch, d, d._cabi.lib()


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _arrays(torch, ld, ny, seed, offset=0, lo=-0.5):
    """(in, out_plain, out_resid) device arrays of ny x ld; `offset` elements into a larger allocation (1: 8 bytes off 16)"""
    rng = np.random.default_rng(seed)
    h = rng.random((ny, ld)) + lo
    base = [torch.empty(ld * ny + 2, dtype=torch.float64, device="cuda") for _ in range(3)]
    a, b, c = (t[offset:offset + ld * ny].view(ny, ld) for t in base)
    a.copy_(torch.from_numpy(h))
    b.fill_(SENT)
    c.fill_(SENT)
    return h, a, b, c, base


def _resid(L, D, a, out, ld, ny, box, norm, res, stream=None):
    D._cabi.check(L.dlesm_stencil5_resid_f64(_ptr(a), _ptr(out), ld, ny, *box, norm, _ptr(res), stream))


def _plain(L, D, a, out, ld, ny, box):
    D._cabi.check(L.dlesm_stencil5_f64(_ptr(a), _ptr(out), ld, ny, *box, None))


def _want(h_in, h_out, box):
    xs, xe, ys, ye = box
    return (h_out - h_in)[ys - 1:ye, xs - 1:xe]


def _cases():
    out = []
    for ld, ny in ((256, 12), (131, 12)):                  # DL_ESM_ALIGNMENT = 64 / unset (an odd pitch)
        for k in range(16):
            xs = 2 + k
            out.append((ld, ny, xs, min(ld - 1, xs + 140 - 3 * k), 2, ny - 1))
        out += [(ld, ny, 2, ld - 1, 5, 5), (ld, ny, 37, 37, 2, ny - 1), (ld, ny, 19, 19, 7, 7), (ld, ny, ld - 1, ld - 1, 2, 3)]
    return out


@pytest.mark.parametrize("offset", [0, 1], ids=["base16", "base8"])
@pytest.mark.parametrize("case", _cases(), ids=lambda c: "x".join(map(str, c)))
def test_out_is_the_plain_step_and_max_is_exact(T, case, offset):
    torch, D, L = T
    ld, ny, *box = case
    h, a, b, c, _keep = _arrays(torch, ld, ny, sum(case) + offset, offset)
    res = torch.full((3,), 3.0, dtype=torch.float64, device="cuda")
    _plain(L, D, a, b, ld, ny, box)
    for norm in (MAX, SUMSQ):                                 # max into res[0], the sum into res[1]
        c.fill_(SENT)
        _resid(L, D, a, c, ld, ny, box, norm, res[norm:])
        torch.cuda.synchronize()
        assert torch.equal(b, c), norm
    got = res.cpu().numpy()
    assert got[2] == 3.0                                      # nothing but *result_dev written
    d = _want(h, b.cpu().numpy(), box)
    assert got[0] == np.max(np.abs(d))
    want = math.fsum((d * d).ravel())
    assert abs(got[1] - want) <= 1e-12 * want, (got[1], want)


def test_max_is_exact_on_ieee_specials(T):
    torch, D, L = T
    ld, ny = 200, 40
    box = (2, 199, 2, 39)
    rng = np.random.default_rng(7)
    h = rng.random((ny, ld)) * 5e-310                         # subnormals
    h[::3, ::5] = 0.0
    h[1::4, 2::7] = -0.0
    h[10, 50] = np.inf
    h[30, 150] = -np.inf
    h[20, 100] = 1e300
    h[21, 101] = -1e300
    for specials, want_nan in ((h, False), (None, True)):
        arr = h.copy()
        if specials is None:
            arr[25, 60] = np.nan
        a = torch.from_numpy(arr).cuda()
        b = torch.full((ny, ld), SENT, dtype=torch.float64, device="cuda")
        res = torch.empty(1, dtype=torch.float64, device="cuda")
        _resid(L, D, a, b, ld, ny, box, MAX, res)
        torch.cuda.synchronize()
        with np.errstate(invalid="ignore", over="ignore"):
            want = np.max(np.abs(_want(arr, b.cpu().numpy(), box)))
        got = float(res)
        if want_nan:
            assert math.isnan(got) and math.isnan(want)
        else:
            assert got == want and got == math.inf, (got, want)
    # subnormals and signed zeros only: the max is a subnormal, and `out` is the oracle's (no flush to zero anywhere)
    sub = rng.random((ny, ld)) * 4e-320
    sub[::3, ::5] = 0.0
    sub[1::4, 2::7] = -0.0
    sub[17, 80] = -3e-310
    a = torch.from_numpy(sub).cuda()
    b = torch.full((ny, ld), SENT, dtype=torch.float64, device="cuda")
    res = torch.empty(1, dtype=torch.float64, device="cuda")
    _resid(L, D, a, b, ld, ny, box, MAX, res)
    torch.cuda.synchronize()
    want_out = np.full((ny, ld), SENT)
    O.jacobi5(sub, want_out, ld, *box)
    got_out = b.cpu().numpy()
    assert np.array_equal(got_out, want_out)
    want = np.max(np.abs(_want(sub, want_out, box)))
    assert 0.0 < want < 2.2250738585072014e-308                 # a subnormal
    assert float(res) == want, (float(res), want)
    # one NaN cell in a big box of zeros: only its wave tile sees it
    a = torch.zeros((ny, ld), dtype=torch.float64, device="cuda")
    a[33, 177] = float("nan")
    b = torch.zeros_like(a)
    res = torch.empty(1, dtype=torch.float64, device="cuda")
    _resid(L, D, a, b, ld, ny, box, MAX, res)
    assert math.isnan(float(res))
    a[33, 177] = 0.0
    a[0, 0] = float("nan")                                    # outside the box and its ring: no effect
    _resid(L, D, a, b, ld, ny, box, MAX, res)
    assert float(res) == 0.0


# the library's defaults of the keys this file sets (dlesm_set_tuning returns 0 for a key never set, not its default)
DEFAULT_TUNING = dict(j5_tpb=0, j5_pad_tiles=0, j5_autoshape=1, j5_skew=1, j5_tile_rows=0, j5_use_tuned=1)
TUNINGS = [{}, {"j5_tpb": 2}, {"j5_tpb": 4}, {"j5_tpb": 8}, {"j5_tpb": 16}, {"j5_pad_tiles": 1}, {"j5_autoshape": 0},
           {"j5_skew": 0}, {"j5_tile_rows": 2}, {"j5_tile_rows": 3}]


def _set(L, tune):
    for k, v in {**DEFAULT_TUNING, **tune}.items():
        L.dlesm_set_tuning(k.encode(), v)


@pytest.mark.parametrize("ld,ny,box", [(2112, 300, (2, 2049, 2, 299)), (2051, 203, (5, 2043, 3, 200))],
                         ids=["even", "odd"])
def test_sumsq_bits_do_not_depend_on_the_launch(T, ld, ny, box):
    torch, D, L = T
    h, a, b, c, _keep = _arrays(torch, ld, ny, ld)
    ref = torch.empty(1, dtype=torch.float64, device="cuda")
    _resid(L, D, a, b, ld, ny, box, SUMSQ, ref)
    torch.cuda.synchronize()
    d = _want(h, b.cpu().numpy(), box)
    want = math.fsum((d * d).ravel())
    assert abs(float(ref) - want) <= 1e-12 * want, (float(ref), want)
    bits = ref.clone()

    def again(stream=None):
        r = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
        c.fill_(SENT)
        torch.cuda.synchronize()
        _resid(L, D, a, c, ld, ny, box, SUMSQ, r, stream)
        torch.cuda.synchronize()
        assert torch.equal(c, b)
        return r

    for _ in range(3):
        assert torch.equal(again(), bits)
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        assert torch.equal(again(C.c_void_p(s.cuda_stream)), bits)
    try:
        for tune in TUNINGS:
            _set(L, tune)
            assert torch.equal(again(), bits), tune
        _set(L, {})
        D._cabi.check(L.dlesm_stencil5_autotune_f64(_ptr(a), _ptr(c), ld, ny, *box, None))
        assert torch.equal(again(), bits), "after the planning call"
        _set(L, {"j5_use_tuned": 0})
        assert torch.equal(again(), bits), "j5_use_tuned 0"
    finally:
        _set(L, {})


def test_empty_box_and_refusals(T):
    torch, D, L = T
    ld, ny = 64, 16
    h, a, b, c, _keep = _arrays(torch, ld, ny, 3)
    res = torch.full((1,), 5.0, dtype=torch.float64, device="cuda")
    _resid(L, D, a, b, ld, ny, (10, 9, 2, 15), MAX, res)      # empty: writes 0.0, launches no sweep
    torch.cuda.synchronize()
    assert float(res) == 0.0 and bool((b == SENT).all())
    res.fill_(5.0)
    _resid(L, D, a, b, ld, ny, (2, 63, 9, 8), SUMSQ, res)
    assert float(res) == 0.0 and bool((b == SENT).all())

    def refused(inp, out, box, norm, rp):
        res.fill_(5.0)
        if out is not inp:
            out.fill_(SENT)
        torch.cuda.synchronize()
        rc = L.dlesm_stencil5_resid_f64(_ptr(inp), _ptr(out), ld, ny, *box, norm, rp, None)
        torch.cuda.synchronize()
        assert rc == -1, (rc, box, norm)                      # DLESM_EINVAL
        assert float(res) == 5.0
        return out

    full = (2, 63, 2, 15)
    for box in ((1, 63, 2, 15), (2, 64, 2, 15), (2, 63, 1, 15), (2, 63, 2, 16)):     # the one-cell ring
        assert bool((refused(a, b, box, MAX, _ptr(res)) == SENT).all())
    assert torch.equal(refused(a, a, full, MAX, _ptr(res)), torch.from_numpy(h).cuda())   # in == out
    assert bool((refused(a, b, full, MAX, None) == SENT).all())                           # null result_dev
    for norm in (2, -1):
        assert bool((refused(a, b, full, norm, _ptr(res)) == SENT).all())
    # result_dev inside in or out
    keep_in = a.clone()
    assert bool((refused(a, b, full, MAX, C.c_void_p(a.data_ptr() + 8 * (ld * 5 + 7))) == SENT).all())
    assert torch.equal(a, keep_in)
    b.fill_(SENT)
    rc = L.dlesm_stencil5_resid_f64(_ptr(a), _ptr(b), ld, ny, *full, MAX, C.c_void_p(b.data_ptr() + 8 * (ld * ny - 1)), None)
    torch.cuda.synchronize()
    assert rc == -1 and bool((b == SENT).all())


@pytest.mark.parametrize("rows", [0, 3])        # the planner's height / 3-row tiles (with non-temporal stores at this size)
def test_headline_size(T, rows):
    torch, D, L = T
    _set(L, {"j5_tile_rows": rows})
    try:
        _headline(torch, D, L)
    finally:
        _set(L, {})


def _headline(torch, D, L):
    n = 16384
    ld, ny = (n + 2 + 63) // 64 * 64, n + 2
    box = (2, n + 1, 2, n + 1)
    g = torch.Generator(device="cuda")
    g.manual_seed(16384)
    a = torch.rand((ny, ld), dtype=torch.float64, device="cuda", generator=g)
    b = torch.full((ny, ld), SENT, dtype=torch.float64, device="cuda")
    c = torch.full((ny, ld), SENT, dtype=torch.float64, device="cuda")
    _plain(L, D, a, b, ld, ny, box)
    res = torch.empty(2, dtype=torch.float64, device="cuda")
    for norm in (MAX, SUMSQ):
        c.fill_(SENT)
        _resid(L, D, a, c, ld, ny, box, norm, res[norm:])
        torch.cuda.synchronize()
        assert torch.equal(b, c), norm
        if norm == MAX:
            d = (b - a)[1:n + 1, 1:n + 1]
            assert float(res[0]) == float(d.abs().max())
    d = (b - a)[1:n + 1, 1:n + 1]
    want = float((d * d).sum())
    assert abs(float(res[1]) - want) <= 1e-12 * want, (float(res[1]), want)


def test_max_beyond_2_31_elements(T):
    torch, D, L = T
    n = 46400
    ld, ny = 46464, n + 3
    assert ld * ny > 2 ** 31
    free, _ = torch.cuda.mem_get_info()
    if free < 48e9:
        pytest.skip(f"needs 48 GB of free device memory, {free / 1e9:.0f} GB there")
    box = (2, n + 1, 2, n + 1)
    g = torch.Generator(device="cuda")
    g.manual_seed(4640)
    a = torch.empty((ny, ld), dtype=torch.float64, device="cuda")
    for r0 in range(0, ny, 4096):
        a[r0:r0 + 4096].copy_(torch.rand((min(4096, ny - r0), ld), dtype=torch.float64, device="cuda", generator=g))
    a[n - 1, n - 5] = 3.5                                 # the largest change sits past element 2^31
    b = torch.full((ny, ld), SENT, dtype=torch.float64, device="cuda")
    res = torch.empty(1, dtype=torch.float64, device="cuda")
    _resid(L, D, a, b, ld, ny, box, MAX, res)
    torch.cuda.synchronize()
    m = torch.zeros((), dtype=torch.float64, device="cuda")
    for r0 in range(1, n + 1, 4096):
        r1 = min(r0 + 4096, n + 1)
        m = torch.maximum(m, (b[r0:r1, 1:n + 1] - a[r0:r1, 1:n + 1]).abs().max())
    assert float(res) == float(m) and float(m) > 2.0
    assert bool((b[0] == SENT).all()) and bool((b[n + 1:] == SENT).all()) and bool((b[:, n + 1:] == SENT).all())
    del a, b
    torch.cuda.empty_cache()


def test_laplace_solve_stops_where_the_oracle_does(T):
    torch, D, L = T
    g = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
    g.decompose(64, 32)
    D.grid_init(g, 1.0, 1.0)
    x, y = D.r2d_field(g, D.GO_T_POINTS), D.r2d_field(g, D.GO_T_POINTS)
    D.psy.hash_init(x, 20261016)
    D.psy.hash_init(y, 20261016)
    it = x.internal
    hx, hy = x.get_data(), y.get_data()
    xs, xe, ys, ye = it.xstart, it.xstop, it.ystart, it.ystop
    steps, r = 0, math.inf
    want_steps, wr = 0, math.inf
    while wr > 1e-9:                                       # the oracle's loop, numpy max norm
        O.jacobi5(hx, hy, g.nx, xs, xe, ys, ye)
        wr = float(np.max(np.abs(hy - hx)[ys - 1:ye, xs - 1:xe]))
        hx, hy = hy, hx
        want_steps += 1
        assert want_steps < 20000
    src, dst = x, y
    while r > 1e-9:
        r = D.psy.invoke_jacobi5_residual(dst, src, "max")
        src, dst = dst, src
        steps += 1
        assert steps <= want_steps
    assert steps == want_steps and r == wr
    assert np.array_equal(src.get_data(), hx)
