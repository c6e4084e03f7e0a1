"""CPU tests of the restatements of the model's output fields (tests/flow_output_numpy.py): the
whole-array and the scalar evaluation agree bit for bit (any NaN equal to any NaN) on the plain and the special-value case of
flow_output_cases at its three shapes, in SET and in ADD, for every selection of outputs the GPU tests use; a census asserts
that the inputs reach every branch of the rule; what land holds changes no written bit; a uniform flow on an all-wet patch
gives UT = a, VT = b and VORT = 0.0 exactly; four ADD calls with weight 1/4 into zeroed arrays equal one SET call bit for bit
(the sign of a zero apart when the arrays are zeroed with +0.0).  No tolerance anywhere."""
import numpy as np
import pytest

import flow_output_cases as OC
import flow_output_numpy as ON

KINDS = ["special", "plain"]
# wet / corner true / corner false / land to the west over each shape's box, counted on the masks of flow_courant_cases
POPULATION = {
    ("plain", 260): (1428, 623, 805, 299), ("special", 260): (1479, 689, 790, 325),
    ("plain", 131): (557, 231, 326, 133), ("special", 131): (648, 362, 286, 104),
    ("plain", 130): (295, 121, 174, 62), ("special", 130): (387, 227, 160, 54),
}


@pytest.mark.parametrize("mode", [ON.SET, ON.ADD])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ld,ny,box", OC.SHAPES)
def test_the_two_restatements_agree(ld, ny, box, kind, mode):
    tm, A = OC.host(kind, ld, ny)
    for sel in OC.SELECTIONS:
        want = OC.reference(kind, ld, ny, box, mode, sel)
        got = OC.outputs(tm.shape, sel)
        for _ in range(2 if mode == ON.ADD else 1):
            ON.flow_output_scalar(mode, OC.WEIGHT, box, tm, *OC.inputs_for(A, sel), got)
        for k in range(ON.COUNT):
            assert (got[k] is None) == (want[k] is None) == (k not in sel)
            if k in sel:
                assert ON.same(got[k], want[k]), (sel, ON.NAMES[k], np.argwhere(got[k] != want[k])[:6].tolist())
                w = ON.written(tm, box, k)
                assert (want[k][~w] == OC.SENTINEL).all() and w.any()
        # an input the selection does not read, filled with NaN instead of left out, changes nothing
        nan = OC.outputs(tm.shape, sel)
        for _ in range(2 if mode == ON.ADD else 1):
            ON.flow_output(mode, OC.WEIGHT, box, tm, *OC.inputs_for(A, sel, "nan"), nan)
        for k in sel:
            assert ON.same(nan[k], want[k]), (sel, k)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ld,ny,box", OC.SHAPES)
def test_census_the_inputs_reach_every_branch(ld, ny, box, kind):
    import flow_courant_cases as FC
    tm, A = OC.host(kind, ld, ny)
    assert np.array_equal(tm, FC.host(kind, ld, ny)[0])           # the masks the populations were counted on
    wet, corner, no_corner, west_land, open_pair = OC.census(tm, box)
    print(kind, ld, ny, wet, corner, no_corner, west_land, open_pair)
    assert (wet, corner, no_corner, west_land) == POPULATION[(kind, ld)]
    assert corner >= 100 and no_corner >= 100 and west_land >= 50 and wet == corner + no_corner
    assert open_pair >= 1                                          # VORT reads a face between two open cells as it is
    S = ON._view(box)
    w = S(tm) > 0
    for di, dj in ((1, 0), (-1, 0), (0, 1), (0, -1)):              # every face switch both ways, an open neighbour too
        t = S(tm, di, dj)[w]
        assert (t == 0).sum() >= 20 and (t > 0).sum() >= 20 and (t < 0).sum() >= 10
    ne = S(tm, 1, 1)[w & (S(tm, 1, 0) != 0) & (S(tm, 0, 1) != 0)]
    assert (ne == 0).sum() >= 10                                   # corner fails on the north-east cell alone
    for n in OC.ARRAYS:
        assert np.isfinite(A[n]).all() == (kind == "plain") or n not in ("un", "vn"), n
    if kind == "plain":                                            # the metrics: non-uniform, 900 .. 1100
        for n in ("dx_v", "dy_u"):
            assert 900.0 <= A[n].min() < 920.0 and 1080.0 < A[n].max() <= 1100.0, n
    else:
        want = OC.reference(kind, ld, ny, box, ON.SET)
        for k in (ON.UT, ON.VT, ON.SPEED, ON.KE, ON.VORT):
            v = want[k][ON.written(tm, box, k)]
            assert np.isinf(v).any() and (np.isnan(v).any() or k == ON.UT), ON.NAMES[k]
        assert (want[ON.SPEED][ON.written(tm, box, ON.SPEED)] == 0.0).any()


@pytest.mark.parametrize("mode", [ON.SET, ON.ADD])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ld,ny,box", OC.SHAPES)
def test_what_land_holds_changes_no_written_bit(ld, ny, box, kind, mode):
    tm, A = OC.host(kind, ld, ny)
    A2 = OC.land_overwritten(tm, A)
    assert np.isnan(A2["un"]).sum() > 100 and np.isnan(A2["vn"]).sum() > 100 and (A2["dx_v"] == -3.0).sum() > 50
    got = OC.outputs(tm.shape, OC.ALL)
    for _ in range(2 if mode == ON.ADD else 1):
        ON.flow_output(mode, OC.WEIGHT, box, tm, *[A2[n] for n in OC.ARRAYS], got)
    want = OC.reference(kind, ld, ny, box, mode)
    for k in range(ON.COUNT):
        assert ON.same(got[k], want[k]), ON.NAMES[k]


def test_uniform_flow_on_an_all_wet_patch():
    ld, ny, box = 40, 12, (2, 39, 2, 11)
    rng = np.random.default_rng(5)
    tm = np.ones((ny, ld), dtype=np.int32)
    a, b = 0.3, -1.7
    A = {"dx_v": 900.0 + 200.0 * rng.random((ny, ld)), "dy_u": 900.0 + 200.0 * rng.random((ny, ld)),
         "un": np.full((ny, ld), a), "vn": np.full((ny, ld), b), "ht": 10.0 + rng.random((ny, ld)),
         "sshn_t": rng.normal(size=(ny, ld))}
    for fn in (ON.flow_output, ON.flow_output_scalar):
        out = OC.outputs(tm.shape, OC.ALL)
        fn(ON.SET, 0.0, box, tm, *[A[n] for n in OC.ARRAYS], out)
        w = ON.written(tm, box, ON.UT)
        assert w.sum() == 38 * 10 and np.array_equal(w, ON.written(tm, box, ON.VORT))
        assert (out[ON.UT][w] == a).all() and (out[ON.VT][w] == b).all()
        assert (out[ON.VORT][w] == 0.0).all() and not np.signbit(out[ON.VORT][w]).any()
        assert ON.same(out[ON.SSH][w], A["sshn_t"][w])
        assert (out[ON.SPEED][w] == np.sqrt(np.float64(a) * a + np.float64(b) * b)).all()
        for k in range(ON.COUNT):
            assert (out[k][~w] == OC.SENTINEL).all()


@pytest.mark.parametrize("ld,ny,box", OC.SHAPES)
def test_a_mean_of_four_identical_steps_equals_set(ld, ny, box):
    """weight = 1/4 over four steps: v/4 and v/2 are exact, 3v/4 is rounded by at most half an ulp of its own, which is a
    quarter of an ulp of v or a tie that goes to v's even mantissa, so the fourth sum rounds to v again -- unless v/4 is
    subnormal, which the plain case does not hold.  Into arrays of -0.0, the identity of IEEE addition, every bit is SET's;
    into arrays of +0.0 a value of -0.0 comes out as +0.0 (0.0 + -0.0), which is the one difference and none by value."""
    tm, A = OC.host("plain", ld, ny)
    want = OC.reference("plain", ld, ny, box, ON.SET)
    for zero in (-0.0, 0.0):
        out = [np.full(tm.shape, zero) for _ in range(ON.COUNT)]
        for _ in range(4):
            ON.flow_output(ON.ADD, 0.25, box, tm, *[A[n] for n in OC.ARRAYS], out)
        for k in range(ON.COUNT):
            w = ON.written(tm, box, k)
            got, ref = out[k][w], want[k][w]
            if np.signbit(zero):
                assert ON.same(got, ref), ON.NAMES[k]
            else:
                differ = got.view(np.uint64) != ref.view(np.uint64)
                assert (got == ref).all() and (ref[differ] == 0.0).all() and np.signbit(ref[differ]).all(), ON.NAMES[k]
                assert not np.signbit(got[differ]).any()
            assert ON.same(out[k][~w], np.full(int((~w).sum()), zero))
