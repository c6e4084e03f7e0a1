"""CPU tests of the drifter rule on its two restatements (tests/drifter_numpy.py): they agree bit for
bit; one call with nsub = 3 is three calls with nsub = 1; what land holds changes no bit; a uniform flow on a uniform metric
moves a particle h*u/dx per substep exactly; a particle at rest stays; the shared inputs (tests/drifter_cases.py) reach
every status, every entry class and both branches of the midpoint select."""
import numpy as np
import pytest

import drifter_cases as DC
import drifter_numpy as DN


@pytest.mark.parametrize("box", DC.BOXES, ids=str)
@pytest.mark.parametrize("nsub", [1, 3])
def test_the_two_restatements_agree_bit_for_bit(box, nsub):
    px, py, st = DC.reference(box, nsub)
    sx, sy, ss, _ = DC.scalar_reference(box, nsub)
    n = DC.NSCALAR
    assert DN.same(px[:n], sx) and DN.same(py[:n], sy) and (st[:n] == ss).all()
    x0, y0, s0 = DC.particles()
    idle = s0 != DN.ACTIVE
    assert DN.same(px[idle], x0[idle]) and DN.same(py[idle], y0[idle]) and (st[idle] == s0[idle]).all()
    assert len(px) == DC.POOL and idle.sum() > 1000


@pytest.mark.parametrize("box", DC.BOXES, ids=str)
def test_one_call_with_three_substeps_is_three_calls_with_one(box):
    a, b = DC.reference(box, 3), DC.reference(box, 1, calls=3)
    assert DN.same(a[0], b[0]) and DN.same(a[1], b[1]) and (a[2] == b[2]).all()
    one = DC.reference(box, 1)
    assert not DN.same(a[0], one[0])
    px, py, st = (v[:DC.NSCALAR].copy() for v in DC.particles())
    for _ in range(3):
        DN.drifter_step_scalar(DC.H, 1, box, *DC.flow(), px, py, st)
    n = DC.NSCALAR
    assert DN.same(a[0][:n], px) and DN.same(a[1][:n], py) and (a[2][:n] == st).all()


@pytest.mark.parametrize("box", DC.BOXES, ids=str)
def test_the_census_reaches_every_class(box):
    """every status value, every entry class, both branches of the midpoint select and each reason for the fallback; the
    sub-box holds no open cell, so the open classes are the full box's"""
    _, _, st, seen = DC.scalar_reference(box, 3)
    print(box, sorted(seen.items()), np.bincount(st))
    want = {"entry_left", "entry_land", "entry_wet", "mid_used", "mid_outside", "mid_land", "move_left", "move_grounded"}
    if box == DC.BOXES[0]:
        want |= {"entry_open", "mid_open", "move_open"}
        assert set(st.tolist()) == {DN.ACTIVE, DN.LEFT, DN.OPEN, DN.GROUNDED, 7}
    assert want <= set(seen), want - set(seen)
    assert all(seen[k] >= 1 for k in want)
    x0, y0, s0 = DC.particles()
    px, py, _ = DC.reference(box, 3)
    for p, (x, y, s) in enumerate(DC.PLACED):
        if s != DN.ACTIVE:
            assert px[p] == x0[p] == x and py[p] == y0[p] == y and st[p] == s


def test_the_placed_particles_do_what_they_are_placed_for():
    box = DC.BOXES[0]
    px, py, st = DC.reference(box, 1)
    at = {(x, y): p for p, (x, y, s) in enumerate(DC.PLACED) if x == x and s == DN.ACTIVE}
    p = at[(6.3, 15.6)]
    assert (px[p], py[p], st[p]) == (6.3, 15.6, DN.ACTIVE)                   # -0.0 velocities: at rest, bit for bit
    for key in ((9.5, 9.5), (16.8, 14.8)):                                 # GROUNDED by a move: the last wet position
        p = at[key]
        assert (px[p], py[p], st[p]) == (*key, DN.GROUNDED)
    p = at[(24.5, 6.5)]
    assert st[p] == DN.LEFT and px[p] == 28.5                               # Euler: 24.5 + 400 * 10 / 1000 ... by dx_t
    p = at[(24.9, 12.5)]
    assert st[p] == DN.OPEN and 25.0 < px[p] < 26.0 and py[p] == 12.5
    p = at[(6.5, 18.5)]
    assert st[p] == DN.LEFT and np.isnan(px[p])
    for key in ((11.5, 9.5), (17.5, 15.5)):
        assert st[at[key]] == DN.GROUNDED
    assert st[at[(25.5, 9.5)]] == DN.OPEN and st[at[(26.0, 5.5)]] == DN.LEFT
    assert st[at[(2.0, 2.0)]] != DN.LEFT and st[at[(float(np.nextafter(2.0, 0.0)), 5.5)]] == DN.LEFT
    sub = DC.reference(DC.BOXES[1], 1)
    p = at[(20.5, 10.5)]
    assert sub[2][p] == DN.LEFT and sub[0][p] > 21.0 and st[p] != DN.LEFT
    for p, (x, y, s) in enumerate(DC.PLACED):                               # NaN and infinite positions: LEFT, untouched
        if s == DN.ACTIVE and not (np.isfinite(x) and np.isfinite(y)):
            assert st[p] == DN.LEFT and DN.same(px[p:p + 1], np.array([x])) and DN.same(py[p:p + 1], np.array([y]))


def test_what_land_holds_changes_no_bit():
    tm, dx_t, dy_t, un, vn = DC.flow()
    land = tm == 0
    un2, vn2, dx2, dy2 = (a.copy() for a in (un, vn, dx_t, dy_t))
    for a in (un2, vn2, dx2, dy2):
        a[land] = np.nan
    # and the faces that touch land from the wet side: un(i, j) with T(i+1, j) == 0, vn(i, j) with T(i, j+1) == 0
    un2[:, :-1][land[:, 1:]] = np.nan
    vn2[:-1, :][land[1:, :]] = np.nan
    assert np.isnan(un2).sum() > np.isnan(un).sum() + 50
    for box in DC.BOXES:
        want = DC.reference(box, 3)
        px, py, st = (a.copy() for a in DC.particles())
        DN.drifter_step(DC.H, 3, box, tm, dx2, dy2, un2, vn2, px, py, st)
        assert DN.same(px, want[0]) and DN.same(py, want[1]) and (st == want[2]).all()
        n = DC.NSCALAR
        px, py, st = (a[:n].copy() for a in DC.particles())
        DN.drifter_step_scalar(DC.H, 3, box, tm, dx2, dy2, un2, vn2, px, py, st)
        assert DN.same(px, want[0][:n]) and DN.same(py, want[1][:n]) and (st == want[2][:n]).all()


@pytest.mark.parametrize("step", [DN.drifter_step, DN.drifter_step_scalar])
def test_uniform_flow_and_rest(step):
    """u = 0.5, v = -0.25, dx = dy = 1000, h = 250: kx = 0.125 and ky = -0.0625 exactly, and so is every sum below"""
    tm = np.ones((12, 14), dtype=np.int32)
    un, vn = np.full((12, 14), 0.5), np.full((12, 14), -0.25)
    d = np.full((12, 14), 1000.0)
    box = (2, 13, 2, 11)
    px, py, st = np.array([3.5, 7.25]), np.array([8.5, 9.0]), np.zeros(2, dtype=np.int32)
    step(250.0, 5, box, tm, d, d, un, vn, px, py, st)
    assert px.tolist() == [3.5 + 5 * 0.125, 7.25 + 5 * 0.125] and py.tolist() == [8.5 - 5 * 0.0625, 9.0 - 5 * 0.0625]
    assert (st == DN.ACTIVE).all()
    px, py = np.array([3.7, 7.1]), np.array([8.3, 9.9])
    step(250.0, 9, box, tm, d, d, 0.0 * un, -0.0 * vn, px, py, st)
    assert px.tolist() == [3.7, 7.1] and py.tolist() == [8.3, 9.9] and (st == DN.ACTIVE).all()


def test_sampling_restatement():
    px, py, st = DC.particles()
    n = DC.NSCALAR
    f = DC.sample_fields(3)
    out = [np.full(n, DC.SENTINEL) for _ in f]
    box = DC.BOXES[1]
    DN.drifter_sample(box, px[:n], py[:n], st[:n], f, out)
    hit = 0
    for p in range(n):
        ok = st[p] == DN.ACTIVE and DN.inbox(box, px[p], py[p])
        for k in range(3):
            want = f[k][int(np.floor(py[p])) - 1, int(np.floor(px[p])) - 1] if ok else DC.SENTINEL
            assert out[k][p] == want
        hit += ok
    assert 100 < hit < n - 100
