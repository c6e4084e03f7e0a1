"""CPU tests of the restatement of the particle order (tests/particle_order_numpy.py): the array form
(the key rule and numpy's stable argsort) and the scalar bucket loop agree on every shared case; perm is a permutation, the
keys along it do not decrease, equal keys keep ascending indices, the live particles are the first nlive; the positions on and
next to the box's edges and the positions that are not finite fall on the side section 6.17's inbox puts them; the boxes
cost the radix passes the cases count on."""
import numpy as np
import pytest

import particle_order_cases as PC
import particle_order_numpy as PN


@pytest.mark.parametrize("n", PC.NS)
def test_the_two_forms_agree_and_perm_is_the_stable_order(n):
    for boxname, box in PC.BOXES.items():
        ncells = PN.cells(box)[2]
        for dist in PC.DISTS:
            px, py, st = PC.case(dist, boxname, n)
            perm, nlive = PC.reference(dist, boxname, n)
            sperm, snlive = PN.order_scalar(box, px.tolist(), py.tolist(), st.tolist())
            assert np.array_equal(perm, sperm) and nlive == snlive, (dist, boxname)
            assert perm.dtype == np.int32 and np.array_equal(np.sort(perm), np.arange(n)), (dist, boxname)
            key, live = PN.keys(box, px, py, st)
            along = key[perm].astype(np.int64)
            assert (np.diff(along) >= 0).all(), (dist, boxname)
            assert (np.diff(perm)[np.diff(along) == 0] > 0).all(), (dist, boxname)            # stable
            assert nlive == int(live.sum()) and (along[:nlive] < ncells).all() and (along[nlive:] == ncells).all()
            assert live[perm[:nlive]].all() and not live[perm[nlive:]].any()
            assert np.array_equal(perm[nlive:], np.flatnonzero(~live)), (dist, boxname)       # the dead keep their order
            if ncells == 0:
                assert nlive == 0 and np.array_equal(perm, np.arange(n))


def test_the_cases_cover_what_they_claim():
    n = PC.NS[-1]
    for boxname, box in PC.BOXES.items():
        assert PN.passes(box) == PC.PASSES[boxname], boxname
        if boxname == "empty":
            continue
        nlive = {dist: PC.reference(dist, boxname, n)[1] for dist in PC.DISTS}
        assert nlive["alldead"] == 0 and nlive["alllive"] == nlive["onecell"] == nlive["twocells"] == n
        assert nlive["sorted"] == nlive["reverse"] == n
        for dist in ("uniform", "mixed", "specials"):
            assert n // 50 < nlive[dist] < n - n // 50, (dist, boxname)
        key = PN.keys(box, *PC.case("onecell", boxname, n))[0]
        assert (key == key[0]).all()
        key = PN.keys(box, *PC.case("twocells", boxname, n))[0]
        if boxname != "1x1":
            assert (key[0::2] == key[0]).all() and (key[1::2] == 0).all() and key[0] == PN.cells(box)[2] - 1
        key = PN.keys(box, *PC.case("sorted", boxname, n))[0].astype(np.int64)
        assert (np.diff(key) >= 0).all()
        key = PN.keys(box, *PC.case("reverse", boxname, n))[0].astype(np.int64)
        assert (np.diff(key) <= 0).all()
        st = PC.case("mixed", boxname, n)[2]
        assert set(st.tolist()) == {0, 1, 2, 3, 7, -1}
        px, py, _ = PC.case("specials", boxname, n)
        assert np.isnan(px).sum() > 100 and np.isposinf(py).sum() > 100 and np.isneginf(px).sum() > 100
    assert PC.TILE % 256 == 0 and PC.NS[-2] > 3 * PC.TILE and PC.NS[-2] % PC.TILE not in (0, PC.TILE - 1)


def test_edge_positions():
    """x == xstart is in, the last double below xstop + 1 is in, xstop + 1 is out, the last double below xstart is out, NaN
    and both infinities are out -- and none of those is ever cast to an integer"""
    for boxname, box in PC.BOXES.items():
        if boxname == "empty":
            continue
        px, py, st, want = PC.edge_particles(box)
        with np.errstate(all="raise"):
            key, live = PN.keys(box, px, py, st)
            perm, nlive = PN.order(box, px, py, st)
        assert np.array_equal(live, want), boxname
        nxb, nyb, ncells = PN.cells(box)
        assert list(key[:4]) == [0, 0, nxb - 1, (nyb - 1) * nxb] and (key[4:] == ncells).all()
        sperm, snlive = PN.order_scalar(box, px, py, st)
        assert nlive == snlive == 4 and np.array_equal(perm, sperm)
        # a status that is not ACTIVE, whatever it is, is not live
        for other in (1, 2, 3, 7, -1):
            assert PN.order(box, px, py, np.full_like(st, other))[1] == 0


def test_permute_restated():
    perm = np.array([2, 0, 5, -1, 1, 7], dtype=np.int32)
    src, dst = np.arange(10.0, 16.0), np.full(6, -7.0)
    PN.permute(perm, src, dst)
    assert dst.tolist() == [12.0, 10.0, 15.0, -7.0, 11.0, -7.0]
