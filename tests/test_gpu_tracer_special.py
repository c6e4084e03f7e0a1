"""GPU tests (-m gpu) of the three tracer transport entries -- dlesm_tracer_step_f64, dlesm_tracer_step_muscl_f64,
dlesm_tracer_step_hancock_f64 (DESIGN.md sections 6.10-6.12) -- on tracer_cases.special_case: IEEE special values in wet
cells (subnormals, signed zeros, infinities, NaN, 1e300 in the flow, the area and the tracers; h_new == 0 and h_old == 0),
exact ties of the limiter (a == b, a == 0, a == -b, 2|a| == |a+b|/2) and Courant numbers of exactly 0, 1 and one ulp below
1.  tests/test_tracer_special_numpy.py shows on the host that the inputs reach each of these and that NaN is a small share of
what is written.  Every cell of every output equals the array restatement, with the wave tile and with the one-cell-per-thread
kernel (the scheme's HOOK key; 131 is the odd pitch that takes it either way): a limiter's select compiled to a minimum
instruction, a comparison inverted, or NaN handling relaxed by a build flag changes these bits.

The comparator is momentum_numpy.same -- bit for bit, any NaN equal to any NaN: the sign and payload of a generated NaN are
not specified and differ between x86 and the GPU."""
import ctypes as C

import numpy as np
import pytest

import momentum_numpy as M
import tracer_cases as TC
from nemolite_boxes import _dev

pytestmark = pytest.mark.gpu

# upwind and limited: section 6.10's rdt; time-centred: also the rdt at which the random faces pass a Courant number of 1
CASES = [(s, r) for s in TC.SCHEMES for r in ((TC.RDT, TC.RDT_BIG) if s == "hancock" else (TC.RDT,))]


@pytest.fixture(scope="module")
def D():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    import dl_esm_inf_amd as d
    torch.cuda.set_device(0)
    d.parallel_init(0, 1)
    return d


def _p(t):
    return C.c_void_p(t.data_ptr())


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _call(D, entry, rdt, ld, ny, box, tmd, dev, ci, co):
    """the C entry `entry` on device tensors, on the null stream; returns its code"""
    return getattr(D._cabi.lib(), entry)(rdt, ld, ny, *box, _p(tmd), _p(dev["area_t"]), *[_p(dev[n]) for n in TC.FLOW],
                                         _ptrs(ci), _ptrs(co), len(ci), None)


def _check(D, scheme, rdt, ld, ny, box, kernel, k):
    """one call with the first k tracers of the shape's special case against the array restatement in every cell of every
    output; the inputs keep their bits; returns (tm, outputs)"""
    import torch
    entry, hook = TC.SCHEMES[scheme][:2]
    tm, area_t, H, c_in, c_out = TC.special_host(ld, ny, rdt)
    want = TC.special_reference(scheme, ld, ny, box, rdt, k)
    dev = _dev(torch, {"area_t": area_t, **H}, 0)
    ci = list(_dev(torch, {str(n): a for n, a in enumerate(c_in[:k])}, 0).values())
    co = list(_dev(torch, {str(n): a for n, a in enumerate(c_out[:k])}, 0).values())
    tmd = torch.from_numpy(tm).cuda()
    L = D._cabi.lib()
    try:
        L.dlesm_set_tuning(hook.encode(), kernel)
        rc = _call(D, entry, rdt, ld, ny, box, tmd, dev, ci, co)
        assert rc == 0, L.dlesm_last_error()
        torch.cuda.synchronize()
    finally:
        L.dlesm_set_tuning(hook.encode(), 0)
    got = [t.cpu().numpy() for t in co]
    for n in range(k):
        bad = ~((got[n].view(np.uint64) == want[n].view(np.uint64)) | (np.isnan(got[n]) & np.isnan(want[n])))
        where = np.argwhere(bad)[:6]
        assert M.same(got[n], want[n]), (n, int(bad.sum()), where.tolist(), [(got[n][j, i], want[n][j, i]) for j, i in where])
        assert M.same(ci[n].cpu().numpy(), c_in[n]), n
    for n in TC.FLOW:
        assert M.same(dev[n].cpu().numpy(), H[n]), n
    assert M.same(dev["area_t"].cpu().numpy(), area_t)
    assert np.array_equal(tmd.cpu().numpy(), tm)
    return tm, got


@pytest.mark.parametrize("ld,ny,box", TC.SPECIAL_SHAPES)
@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("scheme,rdt", CASES)
def test_special_values_follow_ieee_like_the_cpu(D, scheme, rdt, kernel, ld, ny, box):
    """four tracers: ties of the limiter, specials, subnormal slopes, overflowing fluxes; the written cells hold an infinity,
    a NaN and a subnormal"""
    tm, got = _check(D, scheme, rdt, ld, ny, box, kernel, 4)
    assert TC.holds_specials(got, TC.written(tm, box)) == (True, True, True)


@pytest.mark.parametrize("kernel", [0, 1])
@pytest.mark.parametrize("scheme,rdt", CASES)
def test_special_values_with_one_tracer(D, scheme, rdt, kernel):
    """the same inputs with the first tracer alone: the NT = 1 instantiations"""
    ld, ny, box = TC.SPECIAL_SHAPES[0]
    tm, got = _check(D, scheme, rdt, ld, ny, box, kernel, 1)
    assert (got[0][TC.written(tm, box)] != TC.SENTINEL).any()
