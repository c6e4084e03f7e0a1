"""CPU tests of the three tracer transport rules (DESIGN.md sections 6.10-6.12) on tracer_cases.special_case: IEEE special
values, exact ties of the limiter and Courant numbers of exactly 0, 1 and one ulp below 1, in wet cells.  The array and the
scalar restatement of every scheme agree; a census on the host shows that the inputs reach every edge they were built for;
the written cells hold infinities, NaN and subnormals; and NaN stays a small share of every tracer, so that the GPU test of
the same inputs (tests/test_gpu_tracer_special.py) cannot pass on NaN == NaN.

The comparator is momentum_numpy.same -- bit for bit, any NaN equal to any NaN -- here and in that GPU test only: the sign and
payload of a generated NaN are not specified and differ between x86 and the GPU."""
import numpy as np
import pytest

import momentum_numpy as M
import tracer_cases as TC
import tracer_hancock_numpy as TH
from tracer_numpy import _view

RDTS = [TC.RDT, TC.RDT_BIG]
NAN_CAP = 0.10


def _flow(H):
    return [H[n] for n in TC.FLOW]


@pytest.mark.parametrize("rdt", RDTS)
@pytest.mark.parametrize("ld,ny,box", TC.SPECIAL_SHAPES)
@pytest.mark.parametrize("scheme", list(TC.SCHEMES))
def test_restatements_agree_on_special_values(scheme, ld, ny, box, rdt):
    """whole-array numpy == the scalar loop in every cell of every output; only wet cells of the box are written; they hold
    an infinity, a NaN and a subnormal; at most a tenth of what each tracer's written cells hold is NaN"""
    tm, area_t, H, c_in, c_out = TC.special_host(ld, ny, rdt)
    a = TC.special_reference(scheme, ld, ny, box, rdt)
    b = [x.copy() for x in c_out]
    TC.SCHEMES[scheme][3](rdt, box, tm, area_t, *_flow(H), c_in, b)
    wet = TC.written(tm, box)
    assert wet.sum() > 300
    shares = []
    for n in range(4):
        assert M.same(a[n], b[n]), (n, np.argwhere(~((a[n] == b[n]) | (np.isnan(a[n]) & np.isnan(b[n]))))[:5])
        assert (a[n][~wet] == TC.SENTINEL).all()
        shares.append(float(np.isnan(a[n][wet]).mean()))
    print("%s %dx%d rdt %g: NaN shares of the written cells %s" % (scheme, ld, ny, rdt, " ".join("%.4f" % s for s in shares)))
    assert max(shares) <= NAN_CAP, shares
    assert TC.holds_specials(a, wet) == (True, True, True)


def _tie_census(tm, box, c, axis):
    """counts of the limiter's ties among the slopes of c along `axis` that are switched on in the box: a wet cell between
    two cells that are not land; a = c - c(behind), b = c(ahead) - c"""
    S = _view(box)
    d = (1, 0) if axis == "x" else (0, 1)
    on = (S(tm) > 0) & (S(tm, -d[0], -d[1]) != 0) & (S(tm, *d) != 0)
    a = (S(c) - S(c, -d[0], -d[1]))[on]
    b = (S(c, *d) - S(c))[on]
    return {"a == b != 0": int(((a == b) & (a != 0.0)).sum()), "a == 0": int((a == 0.0).sum()),
            "a == -b != 0": int(((a == -b) & (a != 0.0)).sum()),
            "2|a| == |a+b|/2, a*b > 0": int(((2.0 * np.abs(a) == 0.5 * np.abs(a + b)) & (a * b > 0.0)).sum())}


@pytest.mark.parametrize("rdt", RDTS)
@pytest.mark.parametrize("ld,ny,box", TC.SPECIAL_SHAPES)
def test_the_inputs_reach_the_edges_they_were_built_for(ld, ny, box, rdt):
    """tracer 0 meets every tie of the limiter in x and in y; the Courant numbers of the faces of the box's wet cells hold
    1, one ulp below 1, 0, a NaN and an infinity; h_new == 0 and h_old == 0 occur in written cells; a transport is NaN and
    one is infinite; at the big rdt the random faces still run both branches of the factor"""
    tm, area_t, H, c_in, _ = TC.special_host(ld, ny, rdt)
    for axis in "xy":
        ties = _tie_census(tm, box, c_in[0], axis)
        print("%dx%d rdt %g, ties in %s: %s" % (ld, ny, rdt, axis, ties))
        assert all(v > 0 for v in ties.values()), (axis, ties)
    S = _view(box)
    wet = S(tm) > 0
    with np.errstate(all="ignore"):
        n = np.stack([x[wet] for x in TH.courant(rdt, box, area_t, *_flow(H)[:-1])])
        counts = {"n == 1": int((n == 1.0).sum()), "n == 1 - ulp": int((n == TC.ONE_BELOW).sum()),
                  "n == 0": int((n == 0.0).sum()), "n NaN": int(np.isnan(n).sum()), "n inf": int(np.isinf(n).sum())}
        r = np.stack([((S(H["sshn_u"], d, 0) + S(H["hu"], d, 0)) * S(H["un"], d, 0))[wet] for d in (0, -1)]
                     + [((S(H["sshn_v"], 0, d) + S(H["hv"], 0, d)) * S(H["vn"], 0, d))[wet] for d in (0, -1)])
        counts.update({"h_new == 0": int(((S(H["ht"]) + S(H["ssha"]))[wet] == 0.0).sum()),
                       "h_old == 0": int(((S(H["ht"]) + S(H["sshn_t"]))[wet] == 0.0).sum()),
                       "r NaN": int(np.isnan(r).sum()), "r inf": int(np.isinf(r).sum())})
    print("%dx%d rdt %g: %s" % (ld, ny, rdt, counts))
    assert all(v > 0 for v in counts.values()), counts
    if rdt == TC.RDT_BIG:
        mid, big = TH.face_shares(rdt, box, tm, area_t, *_flow(H))
        print("%dx%d: 0 < n < 1 %.3f, n >= 1 %.3f" % (ld, ny, mid, big))
        assert mid >= 0.10 and big >= 0.10
