"""GPU tests (-m gpu) of the reductions' stream-ordered scratch (scratch_alloc_async, csrc/dlesm_runtime.hip: a pool of the
library's own that keeps its freed blocks) through the synchronous dlesm_field_stats_f64 -- the form the Fortran field_stats
calls, its result record in the scratch too -- on the null stream and on a stream of its own, over boxes that need a larger
block and then fit a kept one again; and calls enqueued back to back on one stream with no synchronisation between them,
which must each leave their own numbers.  Checked against numpy as tests/test_gpu_field_stats.py does."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_field_stats import SENT, T, _call, _check, _dev, _ptr, _want  # noqa: F401  (T: the module's fixture)

pytestmark = pytest.mark.gpu

SIZES = [(64, 6), (2048, 300), (131, 7), (4500, 40), (64, 6)]          # small, larger, odd pitch, larger still, small again


def _case(torch, ld, ny, seed):
    rng = np.random.default_rng(seed)
    h = rng.random((ny, ld)) - 0.5
    hm = rng.integers(-1, 2, size=(ny, ld)).astype(np.int32)
    return h, hm, _dev(torch, h), _dev(torch, hm)


@pytest.mark.parametrize("own_stream", [False, True])
def test_sync_entry_over_growing_boxes(T, own_stream):
    """every call's unmasked and masked numbers are right whether its records fit a kept block or need a new one"""
    torch = T[0]
    s = torch.cuda.Stream() if own_stream else None
    sp = C.c_void_p(s.cuda_stream) if own_stream else None
    for n, (ld, ny) in enumerate(SIZES):
        h, hm, (a, _k1), (m, _k2) = _case(torch, ld, ny, 100 + n)
        torch.cuda.synchronize()                             # the inputs were made on torch's stream
        box = (1, ld, 1, ny)
        for rep in range(2):
            got = _call(T, [a], None, [box], ld, ny, stream=sp, sync=True)
            _check(got[0], _want(h, box), "unmasked %dx%d" % (ld, ny))
            got = _call(T, [a], [m], [box], ld, ny, stream=sp, sync=True)
            _check(got[0], _want(h, box, hm), "masked %dx%d" % (ld, ny))


def test_calls_back_to_back_on_one_stream_share_the_buffer(T):
    """four asynchronous calls of different sizes enqueued on one stream, then one synchronisation: each result is its own
    (the later calls reuse the block the first one gave back, in stream order)"""
    torch, D, L = T
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    cases = [_case(torch, ld, ny, 200 + n) + (ld, ny) for n, (ld, ny) in enumerate(SIZES[1:])]
    res = [torch.full((6,), SENT, dtype=torch.float64, device="cuda") for _ in cases]
    torch.cuda.synchronize()
    # the largest first: what it frees is large enough for every later call
    order = sorted(range(len(cases)), key=lambda k: -cases[k][4] * cases[k][5])
    for k in order:
        h, hm, (a, _k1), (m, _k2), ld, ny = cases[k]
        fp, mp = (C.c_void_p * 1)(a.data_ptr()), (C.c_void_p * 1)(m.data_ptr())
        bx = (D._cabi.Region * 1)(D._cabi.Region(0, 0, 1, ld, 1, ny))
        D._cabi.check(L.dlesm_field_stats_async_f64(fp, mp, bx, 1, ld, ny, _ptr(res[k]), sp))
    s.synchronize()
    for k, (h, hm, _a, _m, ld, ny) in enumerate(cases):
        out = (D._cabi.FieldStats * 1).from_buffer_copy(res[k].cpu().numpy().tobytes())
        _check(out[0].as6(), _want(h, (1, ld, 1, ny), hm), "async %dx%d" % (ld, ny))
