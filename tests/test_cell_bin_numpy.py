"""CPU tests of the cell bin's rule: the two restatements of tests/cell_bin_numpy.py -- the scalar
loop over the slots and the array form the GPU tests compare against -- agree bit for bit on the shared cases; the weights
are such that an error in the order of a sum shows (the same runs added in reversed order, or as one sequential run without
chunks, give other bits); the counts add up to nlive; particles on and next to the edges of a box land in section 6.17's
cell or nowhere; SET and ADD as the restatement applies them; the flag."""
import math

import numpy as np
import pytest

import cell_bin_cases as BC
import cell_bin_numpy as BN
import particle_order_cases as PC
import particle_order_numpy as PN

SMALL = [n for n in BC.NS if n <= 257]
CASES = ([(d, b, n) for n in SMALL for b in BC.BOXNAMES for d in PC.DISTS] +
         [(d, b, 4097) for b in ("1x1", "15x16") for d in PC.DISTS] +
         [("onecell", "15x16", 70001), ("twocells", "256x256", 70001)])
LONG_RUNS = [(d, b, n) for d in ("onecell", "twocells") for b in ("15x16", "256x256") for n in (257, 4097, 70001)]


def test_the_two_restatements_agree():
    for dist, boxname, n in CASES:
        box, P = PC.BOXES[boxname], PC.case(dist, boxname, n)
        perm = PC.reference(dist, boxname, n)[0]
        S, has = BC.reference(dist, boxname, n)
        S2, has2, unordered = BN.sums_scalar(box, *P, perm, [None, BC.weights(n, 1), BC.weights(n, 2)])
        assert unordered == 0 and np.array_equal(has, has2), (dist, boxname, n)
        assert BN.same(S, S2), (dist, boxname, n)
        assert not np.signbit(S[:, ~has]).any() and (S[:, ~has] == 0.0).all()


@pytest.mark.parametrize("dist,boxname,n", LONG_RUNS)
def test_an_error_in_the_order_of_a_sum_would_show(dist, boxname, n):
    """for the long runs the GPU tests use: the rule's sum differs, in at least one cell and for each weight array, from the
    same run added backwards and from one sequential sum without chunks"""
    box, P = PC.BOXES[boxname], PC.case(dist, boxname, n)
    perm = PC.reference(dist, boxname, n)[0]
    skey = BN.slot_keys(box, *P, perm)[0]
    S = BC.reference(dist, boxname, n)[0]
    ncells = PN.cells(box)[2]
    for a in (1, 2):
        sw = BC.weights(n, a)[perm]
        backwards = whole = False
        for c in np.unique(skey[skey < ncells]):
            slots = [int(k) for k in np.flatnonzero(skey == c)]
            rule = BN.run_sum(slots, sw)
            assert rule == S[a, c] and math.copysign(1.0, rule) == math.copysign(1.0, S[a, c])
            rev = None
            for k in reversed(slots):
                rev = float(sw[k]) if rev is None else rev + float(sw[k])
            backwards = backwards or rev != rule
            whole = whole or BN.run_sum(slots, sw, chunk=None) != rule
        assert backwards and whole, (a, backwards, whole)


def test_the_counts_add_up_to_nlive():
    for dist, boxname, n in CASES:
        S, has = BC.reference(dist, boxname, n)
        nlive = PC.reference(dist, boxname, n)[1]
        assert S[0].sum() == nlive and int(has.sum()) == int((S[0] > 0).sum()), (dist, boxname, n)
        assert (S[0] == np.floor(S[0])).all()


def test_edges_land_in_their_cell_or_nowhere():
    for boxname, box in PC.BOXES.items():
        if boxname in ("empty", "4096x4096", "5000x5000"):
            continue
        px, py, st, live = PC.edge_particles(box)
        perm = PN.order(box, px, py, st)[0]
        for form in (BN.sums_scalar, BN.sums_array):
            S, has, unordered = form(box, px, py, st, perm, [None])
            nxb = PN.cells(box)[0]
            want = np.zeros(PN.cells(box)[2])
            for x, y, l in zip(px, py, live):
                if l:
                    want[(math.floor(y) - box[2]) * nxb + (math.floor(x) - box[0])] += 1.0
            assert unordered == 0 and np.array_equal(S[0], want) and S[0].sum() == live.sum() == 4, boxname


def test_set_and_add_as_the_restatement_applies_them():
    boxname, n = "15x16", 257
    box = PC.BOXES[boxname]
    S, has = BC.reference("uniform", boxname, n)
    assert has.any() and not has.all()
    ld, ny = box[1] + 3, box[3] + 2
    f = [np.full((ny, ld), 7.25) for _ in range(3)]
    BN.apply(box, BN.SET, -0.5, S, has, f)
    inside = np.zeros((ny, ld), dtype=bool)
    inside[box[2] - 1:box[3], box[0] - 1:box[1]] = True
    for a in range(3):
        got = f[a][inside]
        assert (f[a][~inside] == 7.25).all() and BN.same(got, -0.5 * S[a])
        assert np.signbit(got[~has]).all() and (got[~has] == 0.0).all()           # alpha * +0.0, one rounding
    g = [np.full((ny, ld), 7.25) for _ in range(3)]
    BN.apply(box, BN.ADD, 0.375, S, has, g)
    BN.apply(box, BN.ADD, 0.375, S, has, g)
    for a in range(3):
        got = g[a][inside]
        assert (g[a][~inside] == 7.25).all() and (got[~has] == 7.25).all()
        assert BN.same(got[has], (7.25 + 0.375 * S[a][has]) + 0.375 * S[a][has])


def test_the_flag():
    boxname, n = "15x16", 257
    box, P = PC.BOXES[boxname], PC.case("reverse", boxname, n)
    assert BN.slot_keys(box, *P, None)[1] == 1 and BN.sums_scalar(box, *P, None, [None])[2] == 1
    perm = PC.reference("reverse", boxname, n)[0].copy()
    assert BN.slot_keys(box, *P, perm)[1] == 0
    perm[5], perm[200] = n, -1
    skey, unordered = BN.slot_keys(box, *P, perm)
    assert unordered == 1 and skey[5] == skey[200] == PN.cells(box)[2]
    sorted_ = PC.case("sorted", boxname, n)
    assert BN.slot_keys(box, *sorted_, None)[1] == 0
