"""CPU tests of the tracer schemes' Courant check as tests/tracer_courant_numpy.py restates it: the
two restatements agree in every member on the special-value and the plain case at the three shapes of tracer_cases, with a
small and a large rdt; the inputs reach every edge of the definition (a census); what land holds changes no member; a face
number of exactly the limit counts and one an ulp below does not; the empty box and the box without a wet cell."""
import math

import numpy as np
import pytest

import tracer_cases as TC
import tracer_courant_cases as CC
import tracer_courant_numpy as CN

RDTS = [TC.RDT, TC.RDT_BIG]


def _both(kind, ld, ny, box, rdt, limits=CC.LIMITS):
    tm, area_t, H = CC.host(kind, ld, ny, rdt)
    a = CC.reference(kind, ld, ny, box, rdt, limits)
    b = CN.tracer_courant_scalar(rdt, box, tm, area_t, *CC.flow(H), *limits)
    return a, b


@pytest.mark.parametrize("rdt", RDTS)
@pytest.mark.parametrize("kind", ["special", "plain"])
@pytest.mark.parametrize("ld,ny,box", TC.SPECIAL_SHAPES)
def test_restatements_agree(ld, ny, box, kind, rdt):
    """whole-array numpy == the scalar loop in every member of the record"""
    a, b = _both(kind, ld, ny, box, rdt)
    print(kind, ld, ny, rdt, a)
    assert CN.same_record(a, b), (a, b)
    xs, xe, ys, ye = box
    tm = CC.host(kind, ld, ny, rdt)[0]
    assert a.wet == int((tm[ys - 1:ye, xs - 1:xe] > 0).sum()) > 0
    assert 0 <= a.face_index < ld * ny and 0 <= a.outflow_index < ld * ny
    assert tm.flat[a.face_index] > 0 and tm.flat[a.outflow_index] > 0


@pytest.mark.parametrize("ld,ny,box", TC.SPECIAL_SHAPES)
def test_census_special(ld, ny, box):
    """the special case holds cells that are `bad`, at both rdt; the maxima stay finite and non-negative"""
    for rdt in RDTS:
        rec = CC.reference("special", ld, ny, box, rdt)
        print(ld, ny, rdt, rec)
        assert rec.invalid > 0
        assert 0.0 <= rec.face_max <= CN.DBL_MAX and 0.0 <= rec.outflow_max <= CN.DBL_MAX


@pytest.mark.parametrize("kind", ["special", "plain"])
@pytest.mark.parametrize("ld,ny,box", TC.SPECIAL_SHAPES)
def test_census_limits(ld, ny, box, kind):
    """cells reach both limits at RDT_BIG; none does at RDT = 600 on the plain case, and there nothing is invalid"""
    big = CC.reference(kind, ld, ny, box, TC.RDT_BIG)
    small = CC.reference(kind, ld, ny, box, TC.RDT)
    print(kind, ld, ny, big, small)
    assert big.face_over > 0 and big.outflow_over > 0
    assert big.face_over < big.wet and big.outflow_over < big.wet
    if kind == "plain":
        assert small.face_over == 0 and small.outflow_over == 0 and small.invalid == 0 and big.invalid == 0
        assert small.face_max < 0.5 and small.outflow_max < 1.0


def _cells(kind, ld, ny, box, rdt):
    tm, area_t, H = CC.host(kind, ld, ny, rdt)
    return CN.cells(rdt, box, tm, area_t, *CC.flow(H))


def test_census_ties_and_faceless_cells():
    """an interior face belongs to two cells: at least one plain case has two wet cells that attain face_max (the record
    then names the lower index); and at least one case has wet cells none of whose faces is switched on"""
    ties = faceless = 0
    for ld, ny, box in TC.SPECIAL_SHAPES:
        for rdt in RDTS:
            wet, m, has_m, o, has_o, bad = _cells("plain", ld, ny, box, rdt)
            rec = CC.reference("plain", ld, ny, box, rdt)
            at = np.argwhere(has_m & (m == rec.face_max))
            ties += len(at) >= 2
            if len(at) >= 2:                                   # argwhere is in index order
                j, i = at[0]
                assert rec.face_index == (box[2] - 1 + j) * ld + (box[0] - 1 + i)
            faceless += int((wet & ~has_m & ~bad).sum())
    print("cases with a tie for face_max: %d; wet cells without a switched-on face: %d" % (ties, faceless))
    assert ties >= 1 and faceless >= 1


@pytest.mark.parametrize("rdt", RDTS)
@pytest.mark.parametrize("kind", ["special", "plain"])
@pytest.mark.parametrize("ld,ny,box", TC.SPECIAL_SHAPES)
def test_land_changes_no_member(ld, ny, box, kind, rdt):
    """NaN in un / vn on every face that touches land and in area_t, ht, sshn_t on every land cell: the same record, from
    both restatements"""
    tm, area_t, H = CC.host(kind, ld, ny, rdt)
    assert (tm == 0).any()
    a2, H2 = CC.land_overwritten(tm, area_t, H)
    assert np.isnan(a2).any() and np.isnan(H2["un"]).any() and np.isnan(H2["vn"]).any() and np.isnan(H2["ht"]).any()
    want = CC.reference(kind, ld, ny, box, rdt)
    assert CN.same_record(CN.tracer_courant(rdt, box, tm, a2, *CC.flow(H2), *CC.LIMITS), want)
    assert CN.same_record(CN.tracer_courant_scalar(rdt, box, tm, a2, *CC.flow(H2), *CC.LIMITS), want)


@pytest.mark.parametrize("ld,ny,box", TC.SPECIAL_SHAPES)
def test_a_face_at_the_limit_counts(ld, ny, box):
    """special_case's patch has unit weights, so a face's Courant number is the magnitude of its velocity: with
    face_limit = 1.0 a cell whose largest face velocity is 1 counts, one whose largest is one ulp below does not"""
    rdt = TC.RDT
    tm, area_t, H = CC.special_host(ld, ny, rdt)
    one = (CC.PROBE[0], CC.PROBE[0], CC.PROBE[1], CC.PROBE[1])
    for fn in (CN.tracer_courant, CN.tracer_courant_scalar):
        r = fn(rdt, one, tm, area_t, *CC.flow(CC.patch_probe(H, 1.0)), 1.0, 1.0)
        assert r.face_max == 1.0 and r.face_over == 1 and r.wet == 1 and r.invalid == 0
        r = fn(rdt, one, tm, area_t, *CC.flow(CC.patch_probe(H, -1.0)), 1.0, 1.0)
        assert r.face_max == 1.0 and r.face_over == 1
        r = fn(rdt, one, tm, area_t, *CC.flow(CC.patch_probe(H, TC.ONE_BELOW)), 1.0, 1.0)
        assert r.face_max == TC.ONE_BELOW and r.face_over == 0 and r.wet == 1 and r.invalid == 0
        # and in the whole box the one face moves the count by one cell per side of the face it touches
        a = fn(rdt, box, tm, area_t, *CC.flow(CC.patch_probe(H, 1.0)), 1.0, 1.0)
        b = fn(rdt, box, tm, area_t, *CC.flow(CC.patch_probe(H, TC.ONE_BELOW)), 1.0, 1.0)
        assert 1 <= a.face_over - b.face_over <= 2


def test_empty_and_all_land_boxes():
    tm, area_t, H = CC.plain_host(130, 9)
    for fn in (CN.tracer_courant, CN.tracer_courant_scalar):
        assert fn(TC.RDT, (9, 8, 2, 5), tm, area_t, *CC.flow(H)) == CN.EMPTY
        assert fn(TC.RDT, (2, 129, 5, 4), tm, area_t, *CC.flow(H)) == CN.EMPTY
        assert fn(TC.RDT, (2, 129, 2, 8), np.zeros_like(tm), area_t, *CC.flow(H)) == CN.EMPTY
        assert fn(TC.RDT, (2, 129, 2, 8), -np.ones_like(tm), area_t, *CC.flow(H)) == CN.EMPTY


def test_rdt_limit_estimate():
    rec = CC.reference("plain", 260, 12, (2, 259, 2, 11), TC.RDT)
    lim = CN.rdt_limit(TC.RDT, rec)
    assert lim == TC.RDT * min(0.5 / rec.face_max, 1.0 / rec.outflow_max) and lim > TC.RDT
    assert CN.rdt_limit(TC.RDT, CN.EMPTY) == math.inf
    # n is linear in rdt up to rounding: at the estimate the maxima sit at their limits within a few ulp
    tm, area_t, H = CC.plain_host(260, 12)
    at = CN.tracer_courant(lim, (2, 259, 2, 11), tm, area_t, *CC.flow(H))
    assert max(at.face_max / 0.5, at.outflow_max / 1.0) == pytest.approx(1.0, rel=8 * 2.0 ** -52)
