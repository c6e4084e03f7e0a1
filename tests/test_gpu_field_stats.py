"""GPU test (-m gpu): dlesm_field_stats_async_f64 / dlesm_field_stats_f64 / dlesm_field_locate_f64 on
whole sentinel-filled arrays, numpy on the host copy as the yardstick.
- min, max, count and nonfinite are exactly numpy's over the box: pitches 256 and 131, box starts at every column mod 16,
  one-row / one-column / one-cell boxes, boxes that touch the array's edges, a base at 16 bytes and 8 bytes off 16, and a
  narrow box of 4200 rows whose 4200 records take two levels of the tree;
- |sum - fsum(x)| <= n 2^-52 fsum(|x|) and |sumsq - fsum(x^2)| <= n 2^-52 fsum(x^2): the worst-case bound of ANY order of
  n - 1 additions (each adds a relative error of at most 2^-53 to a partial sum that is at most fsum(|x|); first order
  (n - 1) 2^-53) with a factor 2 of slack for the higher-order terms; data in [-0.5, 0.5);
- masks of -1 / 0 / 1: only cells > 0 count, whatever lies under the others; an all-dry mask gives the empty result;
- subnormals, signed zeros, infinities, NaNs, an overflowing sum of squares;
- a field's six members keep their bits alone, first of 3, last of 8, across streams, repeats and padding;
- every refusal returns DLESM_EINVAL and writes nothing; nothing but result_dev[0..nfields) is written;
- locate: the first NaN, the lowest index of a tie, masked-out matches, no match;
- 16384^2 against torch, a box of more than 2^31 cells;
- psy.run_health in an open-channel NEMOLite2D loop."""
import ctypes as C
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EINVAL = -1
SENT = -7.25
INF = math.inf


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


def _dev(torch, h, offset=0):
    """h on the device, `offset` elements into a larger allocation (1: a base 8 bytes off 16); (view, keep-alive)"""
    base = torch.empty(h.size + 2, dtype=torch.float64 if h.dtype == np.float64 else torch.int32, device="cuda")
    v = base[offset:offset + h.size].view(h.shape)
    v.copy_(torch.from_numpy(h))
    return v, base


def _call(T, fields, masks, boxes, ld, ny, stream=None, res=None, sync=False):
    """the C entry on device arrays -> list of (min, max, sum, sumsq, count, nonfinite)"""
    torch, D, L = T
    n = len(fields)
    fp = (C.c_void_p * n)(*[f.data_ptr() for f in fields])
    mp = None
    if masks is not None:
        mp = (C.c_void_p * n)(*[None if m is None else m.data_ptr() for m in masks])
    bx = (D._cabi.Region * n)(*[D._cabi.Region(0, 0, *b) for b in boxes])
    if sync:
        out = (D._cabi.FieldStats * n)()
        D._cabi.check(L.dlesm_field_stats_f64(fp, mp, bx, n, ld, ny, out, stream))
        return [out[k].as6() for k in range(n)]
    if res is None:
        res = torch.full((6 * n,), SENT, dtype=torch.float64, device="cuda")
    D._cabi.check(L.dlesm_field_stats_async_f64(fp, mp, bx, n, ld, ny, _ptr(res), stream))
    torch.cuda.synchronize()
    out = (D._cabi.FieldStats * n).from_buffer_copy(res[:6 * n].cpu().numpy().tobytes())
    return [out[k].as6() for k in range(n)]


def _want(h, box, mask=None):
    """numpy over the box -> (min, max, fsum(x), fsum(x*x), count, nonfinite, fsum(|x|), cells summed)"""
    xs, xe, ys, ye = box
    x = h[ys - 1:ye, xs - 1:xe]
    x = x[mask[ys - 1:ye, xs - 1:xe] > 0] if mask is not None else x.ravel()
    fin = np.isfinite(x)
    xf = x[fin]
    with np.errstate(over="ignore"):
        sq = xf * xf
    return (xf.min() if xf.size else INF, xf.max() if xf.size else -INF, math.fsum(xf) if np.isfinite(np.abs(xf).sum()) else None,
            math.fsum(sq) if np.isfinite(sq.sum()) else INF, x.size, int((~fin).sum()), math.fsum(np.abs(xf)), xf.size)


def _check(got, want, what=""):
    mn, mx, s, q, cnt, nf, sabs, n = want
    print(what, "got", got, "want", want)
    assert got[0] == mn and got[1] == mx and got[4] == cnt and got[5] == nf, (what, got, want)
    if s is not None:
        assert abs(got[2] - s) <= n * 2.0 ** -52 * sabs, (what, got[2], s, n * 2.0 ** -52 * sabs)
    if q != INF:
        assert abs(got[3] - q) <= n * 2.0 ** -52 * q, (what, got[3], q, n * 2.0 ** -52 * q)
    else:
        assert got[3] == INF


def _cases():
    out = []
    for ld, ny in ((256, 12), (131, 12)):                  # DL_ESM_ALIGNMENT = 64 / unset (an odd pitch)
        for k in range(16):
            xs = 2 + k
            out.append((ld, ny, xs, min(ld - 1, xs + 140 - 3 * k), 2, ny - 1))
        out += [(ld, ny, 2, ld - 1, 5, 5), (ld, ny, 37, 37, 2, ny - 1), (ld, ny, 19, 19, 7, 7), (ld, ny, ld - 1, ld - 1, 2, 3)]
        # no ring needed: boxes that touch the array's edges
        out += [(ld, ny, 1, ld, 1, ny), (ld, ny, 1, 1, 1, 1), (ld, ny, ld, ld, ny, ny), (ld, ny, 1, ld, 1, 1), (ld, ny, 1, ld, ny, ny),
                (ld, ny, 1, 1, 1, ny), (ld, ny, ld, ld, 1, ny), (ld, ny, ld - 2, ld, 1, ny), (ld, ny, 1, 4, 1, ny), (ld, ny, ld - 4, ld, ny, ny)]
    out.append((4500, 5, 1, 4500, 1, 5))                   # several segments per row, in both lane widths
    out.append((4499, 5, 3, 4499, 1, 5))
    # a two-level tree: one record a row in either lane form, 4200 records a field -- more than one level's 4096 (TREE_CHUNK)
    out.append((6, 4200, 2, 5, 1, 4200))
    return out


@pytest.mark.parametrize("offset", [0, 1], ids=["base16", "base8"])
@pytest.mark.parametrize("case", _cases(), ids=lambda c: "x".join(map(str, c)))
def test_box_shapes_are_exact(T, case, offset):
    """the array is NaN outside the box: one cell read from there would show in every member"""
    torch = T[0]
    ld, ny, *box = case
    xs, xe, ys, ye = box
    rng = np.random.default_rng(sum(case) + offset)
    h = np.full((ny, ld), np.nan)
    h[ys - 1:ye, xs - 1:xe] = rng.random((ye - ys + 1, xe - xs + 1)) - 0.5
    hm = rng.integers(-1, 2, size=(ny, ld)).astype(np.int32)
    a, _k1 = _dev(torch, h, offset)
    m, _k2 = _dev(torch, hm, offset)                        # (a mask 4 bytes off 8 with offset = 1)
    got = _call(T, [a, a], [None, m], [box, box], ld, ny)
    _check(got[0], _want(h, box), "unmasked")
    _check(got[1], _want(h, box, hm), "masked")
    assert got[0][5] == 0 and got[0][4] == (xe - xs + 1) * (ye - ys + 1)


def test_masks(T):
    torch = T[0]
    ld, ny = 300, 40
    box = (3, 290, 2, 39)
    rng = np.random.default_rng(5)
    h = rng.random((ny, ld)) - 0.5
    hm = rng.integers(-1, 2, size=(ny, ld)).astype(np.int32)
    a, _k = _dev(torch, h)
    m, _k2 = _dev(torch, hm)
    ref = _call(T, [a], [m], [box], ld, ny)[0]
    _check(ref, _want(h, box, hm))
    assert 0 < ref[4] < (290 - 3 + 1) * (39 - 2 + 1)
    m4, _k6 = _dev(torch, hm, 1)                            # the mask 4 bytes off 8 under 16-byte field lanes
    assert _call(T, [a], [m4], [box], ld, ny)[0] == ref
    dry = np.argwhere(hm[1:39, 2:290] <= 0)
    planted = h.copy()
    for (j, i), v in zip(dry[[0, 7, len(dry) // 2, -1, -5]], (np.nan, np.inf, 1e300, -np.inf, -1e300)):
        assert hm[j + 1, i + 2] <= 0
        planted[j + 1, i + 2] = v
    b, _k3 = _dev(torch, planted)
    assert _call(T, [b], [m], [box], ld, ny)[0] == ref      # what lies under a non-positive mask changes nothing
    unm = _call(T, [b], None, [box], ld, ny)[0]
    assert unm[5] == 3 and unm[0] == -1e300 and unm[1] == 1e300
    alldry, _k4 = _dev(torch, np.minimum(hm, 0))
    assert _call(T, [b], [alldry], [box], ld, ny)[0] == (INF, -INF, 0.0, 0.0, 0, 0)
    allwet, _k5 = _dev(torch, np.full((ny, ld), 3, dtype=np.int32))
    assert _call(T, [a], [allwet], [box], ld, ny)[0][4] == (290 - 3 + 1) * (39 - 2 + 1)
    # masks[k] == NULL inside a mask list: that field is unmasked
    two = _call(T, [a, a], [m, None], [box, box], ld, ny)
    assert two[0] == ref and two[1] == _call(T, [a], None, [box], ld, ny)[0]


def test_ieee_specials(T):
    torch = T[0]
    ld, ny = 200, 40
    box = (2, 199, 2, 39)
    n = 198 * 38
    rng = np.random.default_rng(7)
    h = (rng.random((ny, ld)) - 0.5) * 1e-309                # subnormals of both signs
    h[::3, ::5] = 0.0
    h[1::4, 2::7] = -0.0
    a, _k = _dev(torch, h)
    got = _call(T, [a], None, [box], ld, ny)[0]
    want = _want(h, box)
    _check(got, want)
    assert got[0] == want[0] and got[1] == want[1] and 0.0 < got[1] < 2.2250738585072014e-308 and got[5] == 0
    z = np.zeros((ny, ld))
    z[5::2, 3::2] = -0.0
    a, _k = _dev(torch, z)
    got = _call(T, [a], None, [box], ld, ny)[0]
    assert got[0] == 0.0 and got[1] == 0.0 and got[2] == 0.0 and got[3] == 0.0 and got[4:] == (n, 0)
    # infinities and NaNs are counted, and are absent from min, max and the sums
    h = rng.random((ny, ld)) - 0.5
    clean = _want(h, box)
    spec = h.copy()
    cells = [(10, 50, np.inf), (30, 150, -np.inf), (20, 100, np.nan), (20, 101, -np.nan), (38, 198, np.nan), (1, 1, np.inf)]
    for j, i, v in cells:
        spec[j, i] = v
    spec[0, 0] = np.nan                                     # outside the box
    a, _k = _dev(torch, spec)
    got = _call(T, [a], None, [box], ld, ny)[0]
    want = _want(spec, box)
    _check(got, want)
    assert got[5] == len(cells) and got[4] == n and math.isfinite(got[2]) and got[0] >= -0.5 and got[1] < 0.5
    assert abs(got[2] - (clean[2] - sum(h[j, i] for j, i, _ in cells))) < 1e-9
    a, _k = _dev(torch, np.full((ny, ld), np.nan))
    assert _call(T, [a], None, [box], ld, ny)[0] == (INF, -INF, 0.0, 0.0, n, n)
    # SUM x*x overflows, nothing else does
    big = (rng.random((ny, ld)) + 0.5) * 1e200
    a, _k = _dev(torch, big)
    got = _call(T, [a], None, [box], ld, ny)[0]
    want = _want(big, box)
    assert want[3] == INF
    _check(got, want)
    assert got[3] == INF and math.isfinite(got[2]) and got[5] == 0


def test_a_fields_numbers_do_not_depend_on_the_call(T):
    torch = T[0]
    ld, ny = 2112, 60
    rng = np.random.default_rng(11)
    boxes = [(2, 2049, 2, 59), (3, 2049, 2, 59), (2, 2049, 3, 59), (1, 2112, 1, 60), (700, 705, 9, 9), (2, 2049, 2, 59),
             (5, 4, 2, 59), (9, 1999, 30, 31)]
    hs = [rng.random((ny, ld)) - 0.5 for _ in range(8)]
    hm = rng.integers(-1, 2, size=(ny, ld)).astype(np.int32)
    hs[2][17, 170] = np.nan
    dev = [_dev(torch, h) for h in hs]
    A = [d[0] for d in dev]
    m, _k = _dev(torch, hm)
    masks = [None, m, None, m, None, None, m, m]
    alone = [_call(T, [A[k]], [masks[k]], [boxes[k]], ld, ny)[0] for k in range(8)]
    for k in range(8):                                      # different boxes per field: each field its own numbers
        _check(alone[k], _want(hs[k], boxes[k], hm if masks[k] is not None else None), f"field {k}")
    assert alone[6] == (INF, -INF, 0.0, 0.0, 0, 0)          # an empty box
    assert alone[0] != alone[5] and alone[2][5] == 1
    assert _call(T, A, masks, boxes, ld, ny) == alone
    for k in (0, 1, 7):
        first3 = _call(T, [A[k], A[3], A[4]], [masks[k], masks[3], masks[4]], [boxes[k], boxes[3], boxes[4]], ld, ny)
        assert first3[0] == alone[k] and first3[1:] == [alone[3], alone[4]]
        others = [j for j in range(8) if j != k]
        last8 = _call(T, [A[j] for j in others] + [A[k]], [masks[j] for j in others] + [masks[k]],
                      [boxes[j] for j in others] + [boxes[k]], ld, ny)
        assert last8[7] == alone[k] and last8[:7] == [alone[j] for j in others]
    for _ in range(3):
        assert _call(T, A[:3], masks[:3], boxes[:3], ld, ny) == alone[:3]
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        assert _call(T, A[:3], masks[:3], boxes[:3], ld, ny, stream=C.c_void_p(s.cuda_stream)) == alone[:3]
    assert _call(T, A[:3], masks[:3], boxes[:3], ld, ny, sync=True) == alone[:3]     # the synchronous entry: the same bits
    # other padding: the cells outside the box hold something else
    for k, pad in ((0, SENT), (1, np.nan), (7, 1e300)):
        xs, xe, ys, ye = boxes[k]
        p = np.full((ny, ld), pad)
        p[ys - 1:ye, xs - 1:xe] = hs[k][ys - 1:ye, xs - 1:xe]
        b, _k2 = _dev(torch, p)
        assert _call(T, [b], [masks[k]], [boxes[k]], ld, ny)[0] == alone[k], k


def test_refusals_and_nothing_else_written(T):
    torch, D, L = T
    ld, ny = 64, 16
    h = np.random.default_rng(3).random((ny, ld)) - 0.5
    a, _k = _dev(torch, h)
    keep = a.clone()
    res = torch.full((6 * 9,), SENT, dtype=torch.float64, device="cuda")
    Reg = D._cabi.Region
    full = (1, ld, 1, ny)

    def rc_of(nf, fields, boxes, rp, stream=None):
        fp = (C.c_void_p * max(1, len(fields)))(*fields)
        bx = (Reg * max(1, len(boxes)))(*[Reg(0, 0, *b) for b in boxes])
        rc = L.dlesm_field_stats_async_f64(fp, None, bx, nf, ld, ny, rp, stream)
        torch.cuda.synchronize()
        return rc

    p = a.data_ptr()
    assert rc_of(0, [p], [full], _ptr(res)) == EINVAL
    assert rc_of(9, [p] * 9, [full] * 9, _ptr(res)) == EINVAL
    assert rc_of(-1, [p], [full], _ptr(res)) == EINVAL
    assert rc_of(2, [p, None], [full, full], _ptr(res)) == EINVAL                       # a null field
    for box in ((0, ld, 1, ny), (1, ld + 1, 1, ny), (1, ld, 0, ny), (1, ld, 1, ny + 1)):   # a box that does not fit
        assert rc_of(2, [p, p], [full, box], _ptr(res)) == EINVAL, box
    assert rc_of(1, [p], [full], None) == EINVAL                                         # a null result_dev
    assert "result_dev" in D._cabi.last_error()
    # a result_dev range inside a field: its start, its end, and a range that only reaches into the field
    for off in (0, 8 * (ld * 5 + 7), 8 * (ld * ny - 1)):
        assert rc_of(1, [p], [full], C.c_void_p(p + off)) == EINVAL
    sub = a.view(-1)[6:]                                    # (16-byte aligned) field that starts inside a 2-field result range
    assert rc_of(2, [sub.data_ptr(), sub.data_ptr()], [(1, 8, 1, 1)] * 2, C.c_void_p(sub.data_ptr() - 48)) == EINVAL
    assert bool((res == SENT).all()) and torch.equal(a, keep)
    fp = (C.c_void_p * 1)(p)
    out = (D._cabi.FieldStats * 1)()
    assert L.dlesm_field_stats_f64(fp, None, (Reg * 1)(Reg(0, 0, *full)), 1, ld, ny, None, None) == EINVAL
    assert L.dlesm_field_stats_f64(fp, None, (Reg * 1)(Reg(0, 0, 0, ld, 1, ny)), 1, ld, ny, out, None) == EINVAL
    idx = C.c_int64(77)
    assert L.dlesm_field_locate_f64(_ptr(a), None, ld, ny, 1, ld + 1, 1, ny, 0, 0.0, C.byref(idx), None) == EINVAL
    assert L.dlesm_field_locate_f64(_ptr(a), None, ld, ny, *full, 2, 0.0, C.byref(idx), None) == EINVAL and idx.value == 77
    # under stream capture the call is refused before it enqueues anything: the capture stays intact and replays
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    x = torch.zeros(4, device="cuda")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        x.add_(1.0)
        rc = L.dlesm_field_stats_async_f64(fp, None, (Reg * 1)(Reg(0, 0, *full)), 1, ld, ny, _ptr(res), sp)
        rc2 = L.dlesm_field_locate_f64(_ptr(a), None, ld, ny, *full, 0, 0.0, C.byref(idx), sp)
    assert rc == EINVAL and rc2 == EINVAL
    graph.replay()
    torch.cuda.synchronize()
    assert float(x[0]) == 1.0 and bool((res == SENT).all()) and idx.value == 77
    # a good call of 3 fields writes result_dev[0..3) and nothing behind it; the synchronous entry gives the same bits
    res2 = torch.full((6 * 3 + 6,), SENT, dtype=torch.float64, device="cuda")
    got = _call(T, [a, a, a], None, [full, (2, 9, 2, 3), (5, 4, 1, 1)], ld, ny, res=res2)
    assert bool((res2[18:] == SENT).all()) and bool((res2[:18] != SENT).all())
    assert got == _call(T, [a, a, a], None, [full, (2, 9, 2, 3), (5, 4, 1, 1)], ld, ny, sync=True)
    assert got[2] == (INF, -INF, 0.0, 0.0, 0, 0) and torch.equal(a, keep)
    _check(got[0], _want(h, full))


def _locate(T, a, mask, ld, ny, box, what, value=0.0):
    torch, D, L = T
    idx = C.c_int64(-5)
    D._cabi.check(L.dlesm_field_locate_f64(_ptr(a), None if mask is None else _ptr(mask), ld, ny, *box, what, value,
                                           C.byref(idx), None))
    return idx.value


@pytest.mark.parametrize("ld,offset", [(300, 0), (131, 1)])
def test_locate(T, ld, offset):
    torch = T[0]
    ny = 40
    box = (3, ld - 10, 2, 39)
    rng = np.random.default_rng(13)
    h = rng.random((ny, ld)) - 0.5
    h[0, 5] = np.nan                                        # outside the box
    h[7, 1] = np.inf
    a, _k = _dev(torch, h, offset)
    assert _locate(T, a, None, ld, ny, box, 0) == -1
    for j, i in ((30, 20), (12, 100), (12, 40), (25, 3)):   # several NaNs and an infinity: the first in row-major order
        h[j, i] = np.nan
    h[12, 39] = -np.inf
    a, _k = _dev(torch, h, offset)
    assert _locate(T, a, None, ld, ny, box, 0) == 12 * ld + 39
    hm = np.ones((ny, ld), dtype=np.int32)
    hm[12, 39] = 0
    hm[12, 40] = -1
    m, _k2 = _dev(torch, hm, offset)
    assert _locate(T, a, m, ld, ny, box, 0) == 12 * ld + 100          # masked-out matches are skipped
    st = _call(T, [a], [m], [box], ld, ny)[0]
    assert st[5] == 3
    # EQUAL with stats.max: the lowest index of a tie
    h2 = rng.random((ny, ld)) - 0.5
    for j, i in ((33, 9), (20, 110), (20, 64)):
        h2[j, i] = 0.75
    h2[1, 1] = 0.75                                         # row 2, column 2: outside the box (it starts at column 3)
    a, _k = _dev(torch, h2, offset)
    st = _call(T, [a], None, [box], ld, ny)[0]
    assert st[1] == 0.75
    assert _locate(T, a, None, ld, ny, box, 1, st[1]) == 20 * ld + 64
    k = int(np.argmin(h2[1:39, 2:ld - 10].ravel()))         # the box is ld - 12 columns wide
    assert _locate(T, a, None, ld, ny, box, 1, st[0]) == (k // (ld - 12) + 1) * ld + 2 + k % (ld - 12)
    hm = np.ones((ny, ld), dtype=np.int32)
    hm[20, 64] = 0
    m, _k2 = _dev(torch, hm, offset)
    assert _locate(T, a, m, ld, ny, box, 1, 0.75) == 20 * ld + 110
    assert _locate(T, a, None, ld, ny, box, 1, 0.8) == -1   # no match
    assert _locate(T, a, None, ld, ny, (5, 4, 2, 39), 1, 0.75) == -1


def test_headline_size(T):
    torch = T[0]
    n = 16384
    ld, ny = (n + 2 + 63) // 64 * 64, n + 2
    box = (2, n + 1, 2, n + 1)
    g = torch.Generator(device="cuda")
    g.manual_seed(16384)
    a = torch.rand((ny, ld), dtype=torch.float64, device="cuda", generator=g) - 0.5
    a[0, :] = float("nan")                                  # the ring is not read
    a[:, 0] = float("inf")
    a[9000, 777] = float("nan")
    a[16000, 16000] = float("-inf")
    got = _call(T, [a], None, [box], ld, ny)[0]
    x = a[1:n + 1, 1:n + 1]
    fin = torch.isfinite(x)
    xf = torch.where(fin, x, torch.zeros((), dtype=torch.float64, device="cuda"))
    assert got[4] == n * n and got[5] == n * n - int(fin.sum()) == 2
    assert got[0] == float(torch.where(fin, x, torch.full((), 9.0, dtype=torch.float64, device="cuda")).min())
    assert got[1] == float(torch.where(fin, x, torch.full((), -9.0, dtype=torch.float64, device="cuda")).max())
    nsum = n * n - 2
    bound = nsum * 2.0 ** -52 * float(xf.abs().sum())
    print("sum", got[2], float(xf.sum()), "bound", bound)
    assert abs(got[2] - float(xf.sum())) <= bound
    bound = nsum * 2.0 ** -52 * float((xf * xf).sum())
    print("sumsq", got[3], float((xf * xf).sum()), "bound", bound)
    assert abs(got[3] - float((xf * xf).sum())) <= bound
    m = (torch.rand((ny, ld), device="cuda", generator=g) < 0.7).to(torch.int32)
    gm = _call(T, [a, a], [m, None], [box, box], ld, ny)
    assert gm[1] == got
    wet = m[1:n + 1, 1:n + 1] > 0
    assert gm[0][4] == int(wet.sum()) and gm[0][5] == int((wet & ~fin).sum())
    assert gm[0][1] == float(torch.where(wet & fin, x, torch.full((), -9.0, dtype=torch.float64, device="cuda")).max())


def test_box_beyond_2_31_cells(T):
    torch = T[0]
    n = 46400
    ld, ny = 46464, n + 3
    assert n * n > 2 ** 31
    free, _ = torch.cuda.mem_get_info()
    if free < 24e9:
        pytest.skip(f"needs 24 GB of free device memory, {free / 1e9:.0f} GB there")
    box = (2, n + 1, 2, n + 1)
    g = torch.Generator(device="cuda")
    g.manual_seed(4640)
    a = torch.empty((ny, ld), dtype=torch.float64, device="cuda")
    for r0 in range(0, ny, 4096):
        a[r0:r0 + 4096].copy_(torch.rand((min(4096, ny - r0), ld), dtype=torch.float64, device="cuda", generator=g) - 0.5)
    a[n, n] = 3.5                                           # the last cell of the box, past element 2^31
    a[n + 1, 5] = 7.0                                       # behind the box
    a[n, n + 1] = 7.0
    got = _call(T, [a], None, [box], ld, ny)[0]
    assert got[4] == n * n and got[5] == 0 and got[1] == 3.5 and -0.5 <= got[0] < -0.49
    s = sabs = 0.0
    for r0 in range(1, n + 1, 4096):                        # sums of slabs, added on the host
        r1 = min(r0 + 4096, n + 1)
        s += float(a[r0:r1, 1:n + 1].sum())
        sabs += float(a[r0:r1, 1:n + 1].abs().sum())
    assert abs(got[2] - s) <= n * n * 2.0 ** -52 * sabs
    where = _locate(T, a, None, ld, ny, box, 1, got[1])
    assert where == n * ld + n and where > 2 ** 31
    del a
    torch.cuda.empty_cache()


def test_run_health_in_an_open_channel_loop(T):
    """the set-up of test_gpu_open_bc.py::test_open_channel_time_loop (1024 x 256, open first and last columns, a 12 h tide),
    stepped with the separate kernels; run_health every 5 steps on ssha, ua, va under tmask"""
    torch, D, L = T
    nx, ny, steps, rdt, amp = 1024, 256, 20, 20.0, 0.1
    omega = 2.0 * math.pi / (12.0 * 3600.0)
    user = np.ones((ny + 2, nx + 2), dtype=np.int32)
    user[:, 0] = user[:, -1] = 0
    user[:, 1] = user[:, nx] = -1
    user[:2, :] = 0
    user[-2:, :] = 0
    os.environ["DL_ESM_ALIGNMENT"] = "64"
    g = D.grid_type(D.GO_ARAKAWA_C, (1, 1, 2), D.GO_OFFSET_NE)
    g.decompose(nx, ny)
    D.grid_init(g, 1000.0, 1000.0, tmask=user)
    os.environ.pop("DL_ESM_ALIGNMENT", None)
    D.psy.coriolis(g)
    Tp, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
    names = ("ssha", "sshn_t", "sshn_u", "sshn_v", "ssha_u", "ssha_v", "un", "vn", "ua", "va", "ht", "hu", "hv")
    pts = (Tp, Tp, U, V, U, V, U, V, U, V, Tp, U, V)
    F = {k: D.r2d_field(g, p) for k, p in zip(names, pts)}
    for k in ("ht", "hu", "hv"):
        F[k].data.fill_(10.0)
    D.psy.open_boundary(g)
    prm = D.psy.momentum_params(rdt, 0.00015, 50.0, 9.80665)
    mom = ("un", "vn", "ht", "sshn_t", "hu", "sshn_u", "hv", "sshn_v", "ssha_u", "ssha_v")
    tm = g.tmask_device
    htm = g.tmask
    checked = 0
    for step in range(steps):
        ssh_bc = D.psy.tide_ssh(amp, omega, (step + 1) * rdt)
        D.psy.invoke_continuity(F["ssha"], F["sshn_t"], F["sshn_u"], F["sshn_v"], F["hu"], F["hv"], F["un"], F["vn"], rdt)
        D.psy.invoke_next_sshu(F["ssha_u"], F["ssha"])
        D.psy.invoke_next_sshv(F["ssha_v"], F["ssha"])
        D.psy.invoke_momentum(prm, F["ua"], F["va"], *[F[k] for k in mom])
        D.psy.invoke_bc_open(prm, ssh_bc, F["ssha"], F["ua"], F["va"], F["hu"], F["sshn_u"], F["hv"], F["sshn_v"], F["sshn_t"])
        if (step + 1) % 5 == 0:
            flds = [F["ssha"], F["ua"], F["va"]]
            stats = D.psy.run_health(flds, ("ssha", "ua", "va"), masks=tm, max_abs=[5.0, 10.0, 10.0])
            for f, st in zip(flds, stats):
                want = _want(f.get_data(), f.internal.box(), htm)
                _check(st.as6(), want, f"step {step + 1}")
                assert st.nonfinite == 0 and math.isfinite(st.sum) and math.isfinite(st.sumsq) and st.count == want[4] > 0
            checked += 1
        for a, b in (("un", "ua"), ("vn", "va"), ("sshn_t", "ssha"), ("sshn_u", "ssha_u"), ("sshn_v", "ssha_v")):
            F[a], F[b] = F[b], F[a]
    assert checked == 4
    ua = F["ua"]
    st = D.field_stats([F["ssha"], ua, F["va"]], tm)
    assert st[0].max > 0.0                                  # the tide has come in
    # a bound that the field exceeds: the message names the field and the cell of the extreme
    top = D.field_stats([F["ssha"]], tm)[0]
    value = top.max if abs(top.max) >= abs(top.min) else top.min
    cell = D.field_locate(F["ssha"], "equal", value, tm)
    with pytest.raises(D.DlesmError) as e:
        D.psy.run_health([F["ssha"], ua, F["va"]], ("ssha", "ua", "va"), masks=tm, max_abs=[abs(value) / 2, None, None])
    assert "field ssha" in str(e.value) and f"(i, j) = ({cell[0]}, {cell[1]})" in str(e.value)
    # a NaN in one wet cell of ua: the next call raises, naming ua and that (i, j); a NaN on land does not
    it = ua.internal
    i, j = it.xstart + 300, it.ystart + 100
    assert htm[j - 1, i - 1] > 0
    land = np.argwhere(htm[it.ystart - 1:it.ystop, it.xstart - 1:it.xstop] <= 0)[0]
    ua.data[it.ystart - 1 + int(land[0]), it.xstart - 1 + int(land[1])] = float("nan")
    assert D.psy.run_health([F["ssha"], ua, F["va"]], ("ssha", "ua", "va"), masks=tm)[1].nonfinite == 0
    ua.data[j - 1, i - 1] = float("nan")
    ua.data[j + 20, i - 50] = float("nan")                  # a later one
    with pytest.raises(D.DlesmError) as e:
        D.psy.run_health([F["ssha"], ua, F["va"]], ("ssha", "ua", "va"), masks=tm)
    assert "field ua" in str(e.value) and f"(i, j) = ({i}, {j})" in str(e.value) and "rank 1" in str(e.value), str(e.value)
    assert D.field_locate(ua, "nonfinite", mask=tm) == (i, j) and D.field_locate(F["va"], "nonfinite", mask=tm) is None
