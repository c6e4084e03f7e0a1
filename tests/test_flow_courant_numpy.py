"""CPU tests of the flow step's stability check as tests/flow_courant_numpy.py restates it: the two
restatements agree in every member on the special-value and the plain case at the three shapes of flow_courant_cases, with a
small and a large rdt and two sets of limits; the inputs reach every edge of the definition (a census): both sides of each
a >= b select, a bad cell of each kind, a cell exactly at each limit, a tie resolved to the lower index; what land holds
changes no member; visc == 0; the empty box and the box without a wet cell."""
import math

import numpy as np
import pytest

import flow_courant_cases as FC
import flow_courant_numpy as FN

RDTS = [FC.RDT, FC.RDT_BIG]


def _both(kind, ld, ny, box, rdt, limits=FC.LIMITS, visc=FC.VISC):
    tm, A = FC.host(kind, ld, ny)
    a = FC.reference(kind, ld, ny, box, rdt, limits, visc)
    b = FN.flow_courant_scalar(rdt, FC.G, visc, box, tm, *FC.arrays(A), *limits)
    return a, b


@pytest.mark.parametrize("limits", [FC.LIMITS, FC.LIMITS_BIG])
@pytest.mark.parametrize("rdt", RDTS)
@pytest.mark.parametrize("kind", ["special", "plain"])
@pytest.mark.parametrize("ld,ny,box", FC.SHAPES)
def test_restatements_agree(ld, ny, box, kind, rdt, limits):
    """whole-array numpy == the scalar loop in every member of the record"""
    a, b = _both(kind, ld, ny, box, rdt, limits)
    print(kind, ld, ny, rdt, a)
    assert FN.same_record(a, b), (a, b)
    xs, xe, ys, ye = box
    tm = FC.host(kind, ld, ny)[0]
    assert a.wet == int((tm[ys - 1:ye, xs - 1:xe] > 0).sum()) > 0
    for at in a[4:8]:
        assert 0 <= at < ld * ny and tm.flat[at] > 0
    assert 0.0 < a.depth_min < math.inf and a.gravity_max > 0.0 and a.viscous_max > 0.0


def _cells(kind, ld, ny, box, rdt, visc=FC.VISC):
    tm, A = FC.host(kind, ld, ny)
    return FN.cells(rdt, FC.G, visc, box, tm, *FC.arrays(A))


@pytest.mark.parametrize("kind", ["special", "plain"])
@pytest.mark.parametrize("ld,ny,box", FC.SHAPES)
def test_census_selects(ld, ny, box, kind):
    """both sides of um = a1 >= a2 ? a1 : a2 and of vm = a3 >= a4 ? a3 : a4, equality included, among the sound wet cells"""
    c = _cells(kind, ld, ny, box, FC.RDT)
    ok = c["wet"] & ~c["bad"]
    a1, a2, a3, a4 = c["a"]
    for p, q in ((a1, a2), (a3, a4)):
        assert (ok & (p > q)).any() and (ok & (p < q)).any() and (ok & (p == q)).any()


@pytest.mark.parametrize("ld,ny,box", FC.SHAPES)
def test_census_bad_cells(ld, ny, box):
    """the special case holds, in wet cells of the box: d < 0, d == 0, a NaN d, an infinite ix (dx_t == 0), an infinite and a
    NaN face velocity on a switched-on face (one of them towards an open cell), and sound cells beside them"""
    tm, A = FC.special_host(ld, ny)
    S = FN._view(box)
    c = _cells("special", ld, ny, box, FC.RDT_BIG)
    wet, bad = c["wet"], c["bad"]
    a = np.stack(c["a"])
    with np.errstate(all="ignore"):
        kinds = {"d < 0": wet & (c["d"] < 0.0), "d == 0": wet & (c["d"] == 0.0), "d NaN": wet & np.isnan(c["d"]),
                 "dx_t == 0": wet & (S(A["dx_t"]) == 0.0), "infinite velocity": wet & np.isinf(a).any(axis=0),
                 "NaN velocity": wet & np.isnan(a).any(axis=0),
                 "infinite velocity on an open face": wet & (S(tm, 1, 0) < 0) & np.isinf(S(A["un"]))}
    print({k: int(v.sum()) for k, v in kinds.items()}, int(bad.sum()), int(wet.sum()))
    for name, cond in kinds.items():
        assert cond.any() and not (cond & ~bad).any(), name
    assert 0 < bad.sum() < wet.sum()
    rec = FC.reference("special", ld, ny, box, FC.RDT_BIG)
    assert rec.invalid == bad.sum() and all(0.0 <= x <= FN.DBL_MAX for x in rec[:4])


@pytest.mark.parametrize("kind", ["special", "plain"])
@pytest.mark.parametrize("ld,ny,box", FC.SHAPES)
def test_census_limits(ld, ny, box, kind):
    """cells on both sides of each of LIMITS_BIG at RDT_BIG; on the plain case none reaches a default limit at RDT and
    nothing is invalid; a cell at exactly each limit counts and none does one ulp beyond"""
    big = FC.reference(kind, ld, ny, box, FC.RDT_BIG, FC.LIMITS_BIG)
    small = FC.reference(kind, ld, ny, box, FC.RDT)
    print(kind, ld, ny, big, small)
    sound = big.wet - big.invalid
    for n in (big.gravity_over, big.advective_over, big.viscous_over, big.shallow):
        assert 0 < n < sound
    if kind == "plain":
        assert small[8:13] == (0, 0, 0, 0, 0) and big.invalid == 0
        assert small.gravity_max < 1.0 and small.advective_max < 1.0 and small.viscous_max < 0.25
    tm, A = FC.host(kind, ld, ny)
    at, beyond = FC.at_the_limits(small)
    for fn in (FN.flow_courant, FN.flow_courant_scalar):
        r = fn(FC.RDT, FC.G, FC.VISC, box, tm, *FC.arrays(A), *at)
        assert min(r.gravity_over, r.advective_over, r.viscous_over, r.shallow) >= 1, r
        r = fn(FC.RDT, FC.G, FC.VISC, box, tm, *FC.arrays(A), *beyond)
        assert (r.gravity_over, r.advective_over, r.viscous_over, r.shallow) == (0, 0, 0, 0), r


@pytest.mark.parametrize("ld,ny,box", FC.SHAPES)
def test_census_ties(ld, ny, box):
    """the special case's patch attains the gravity-wave and the viscous maximum in many cells and the smallest column in
    two: the record names the lowest index of each"""
    rec = FC.reference("special", ld, ny, box, FC.RDT)
    c = _cells("special", ld, ny, box, FC.RDT)
    ok = c["wet"] & ~c["bad"]
    for x, top, index in ((c["gw"], rec.gravity_max, rec.gravity_index), (c["vis"], rec.viscous_max, rec.viscous_index),
                          (c["d"], rec.depth_min, rec.depth_index)):
        at = np.argwhere(ok & (x == top))                   # argwhere is in index order
        assert len(at) >= 2
        assert index == (box[2] - 1 + at[0][0]) * ld + (box[0] - 1 + at[0][1])
    assert rec.depth_min == 5.0e-324


@pytest.mark.parametrize("rdt", RDTS)
@pytest.mark.parametrize("kind", ["special", "plain"])
@pytest.mark.parametrize("ld,ny,box", FC.SHAPES)
def test_land_changes_no_member(ld, ny, box, kind, rdt):
    """NaN in un / vn on every face that touches land, and NaN, infinities, negative numbers in ht, sshn_t, dx_t, dy_t on every
    land cell: the same record, from both restatements"""
    tm, A = FC.host(kind, ld, ny)
    assert (tm == 0).any()
    A2 = FC.land_overwritten(tm, A)
    assert np.isnan(A2["un"]).sum() > np.isnan(A["un"]).sum() and np.isnan(A2["ht"]).any()
    want = FC.reference(kind, ld, ny, box, rdt)
    assert FN.same_record(FN.flow_courant(rdt, FC.G, FC.VISC, box, tm, *FC.arrays(A2)), want)
    assert FN.same_record(FN.flow_courant_scalar(rdt, FC.G, FC.VISC, box, tm, *FC.arrays(A2)), want)


@pytest.mark.parametrize("kind", ["special", "plain"])
def test_no_viscosity(kind):
    """visc == 0: viscous_max == 0.0 at the lowest sound wet cell, no count; the other members as with viscosity"""
    ld, ny, box = FC.SHAPES[0]
    a, b = _both(kind, ld, ny, box, FC.RDT_BIG, visc=0.0)
    assert FN.same_record(a, b)
    with_visc = FC.reference(kind, ld, ny, box, FC.RDT_BIG)
    assert a.viscous_max == 0.0 and a.viscous_over == 0 and a.viscous_index >= 0
    assert a._replace(viscous_max=with_visc.viscous_max, viscous_index=with_visc.viscous_index,
                      viscous_over=with_visc.viscous_over) == with_visc


def test_empty_and_all_land_boxes():
    tm, A = FC.plain_host(130, 9)
    for fn in (FN.flow_courant, FN.flow_courant_scalar):
        assert fn(FC.RDT, FC.G, FC.VISC, (9, 8, 2, 5), tm, *FC.arrays(A)) == FN.EMPTY
        assert fn(FC.RDT, FC.G, FC.VISC, (2, 129, 5, 4), tm, *FC.arrays(A)) == FN.EMPTY
        assert fn(FC.RDT, FC.G, FC.VISC, (2, 129, 2, 8), np.zeros_like(tm), *FC.arrays(A)) == FN.EMPTY
        assert fn(FC.RDT, FC.G, FC.VISC, (2, 129, 2, 8), -np.ones_like(tm), *FC.arrays(A)) == FN.EMPTY
    assert FN.EMPTY == (0.0, 0.0, 0.0, math.inf, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0)


def test_rdt_limit_estimate():
    rec = FC.reference("plain", 260, 12, (2, 259, 2, 11), FC.RDT)
    lim = FN.rdt_limit(FC.RDT, rec)
    assert lim == FC.RDT * min(1.0 / rec.gravity_max, 1.0 / rec.advective_max, 0.25 / rec.viscous_max) and lim > FC.RDT
    assert FN.rdt_limit(FC.RDT, FN.EMPTY) == math.inf
    assert FN.rdt_limit(FC.RDT, rec._replace(viscous_max=0.0, advective_max=0.0)) == FC.RDT * (1.0 / rec.gravity_max)
