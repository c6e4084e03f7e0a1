"""CPU tests of the dispersal rule as tests/dispersal_numpy.py restates it: Philox4x32-10 gives the
published answers; the word -> (-1, 1) map is exact and symmetric; the scalar and the array restatement agree bit for bit;
kh = 0 is the drifter step; one call with nsub = k at tick t is k calls with nsub = 1 at ticks t .. t+k-1; a particle's path
follows its id, not its slot; in still water nobody is GROUNDED; the shared case takes every branch of the kick often enough;
and the cloud of a point release has the variance 2 kh t per axis, a zero mean and uncorrelated axes within five standard
errors."""
from fractions import Fraction

import numpy as np

import dispersal_cases as PC
import dispersal_numpy as PN
import drifter_cases as DC
import drifter_numpy as DN

KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def _same3(a, b, n=None):
    return DN.same(a[0][:n], b[0][:n]) and DN.same(a[1][:n], b[1][:n]) and bool((a[2][:n] == b[2][:n]).all())


def test_philox_gives_the_published_answers():
    for counter, key, want in KNOWN:
        assert PN.philox(counter, key) == want
        got = PN.philox_v(*[np.array([c, c], dtype=np.uint64) for c in counter], *key)
        assert all(g.tolist() == [w, w] for g, w in zip(got, want))
    # one array call over different counters is the scalar call on each
    c0 = np.array([0, 0xffffffff, 0x243f6a88, 7], dtype=np.uint64)
    got = PN.philox_v(c0, 0, 5, 1, 0x34567891, 0xC0FFEE12)
    for k, c in enumerate(c0.tolist()):
        assert tuple(int(g[k]) for g in got) == PN.philox((c, 0, 5, 1), (0x34567891, 0xC0FFEE12))


def test_the_word_map_is_exact_and_symmetric():
    words = [0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]
    for w in words:
        r = PN.sym(w)
        assert Fraction(float(r)) == Fraction(2 * w + 1, 2 ** 32) - 1, w          # the centre of bin w, no rounding
        assert -1.0 < r < 1.0 and r != 0.0
        assert PN.sym(2 ** 32 - 1 - w) == -r
    v = PN.sym_v(np.array(words, dtype=np.uint64))
    assert DN.same(v, np.array([PN.sym(w) for w in words]))
    assert PN.sym(0) == -1.0 + 2.0 ** -32 and PN.sym(2 ** 32 - 1) == 1.0 - 2.0 ** -32
    assert PN.sym(2 ** 31 - 1) == -2.0 ** -32 and PN.sym(2 ** 31) == 2.0 ** -32
    assert float(PN.amplitude(PC.KH, DC.H)) == 300.0


def test_the_two_restatements_agree():
    for box in DC.BOXES:
        for nsub in (1, 3):
            for with_ids in (False, True):
                a, s = PC.reference(box, nsub, with_ids), PC.scalar_reference(box, nsub, with_ids)
                assert _same3(a, s, DC.NSCALAR), (box, nsub, with_ids)
    a, b = PC.reference(DC.BOXES[0], 3, False), PC.reference(DC.BOXES[0], 3, True)
    assert not DN.same(a[0], b[0])                                              # the ids matter
    assert not DN.same(a[0], DC.reference(DC.BOXES[0], 3)[0])                   # ... and so does the kick
    idle = DC.particles()[2] != DN.ACTIVE
    assert DN.same(a[0][idle], DC.particles()[0][idle]) and (a[2][idle] == DC.particles()[2][idle]).all()


def test_kh_zero_is_the_drifter_step():
    for box in DC.BOXES:
        for nsub in (1, 3):
            got = PC.reference(box, nsub, True, kh=0.0)
            assert _same3(got, DC.reference(box, nsub)), (box, nsub)
            assert got[3]["left_by_kick"] == 0 and got[3]["open_by_kick"] == 0
            px, py, st = (a[:DC.NSCALAR].copy() for a in DC.particles())
            PN.dispersal_step_scalar(DC.H, nsub, 0.0, PC.SEED, PC.TICK, box, *DC.flow(), px, py, st)
            assert _same3((px, py, st), DC.scalar_reference(box, nsub)), (box, nsub)


def test_one_call_with_nsub_k_is_k_calls_at_successive_ticks():
    for box in DC.BOXES:
        for with_ids in (False, True):
            assert _same3(PC.reference(box, 3, with_ids), PC.reference(box, 1, with_ids, calls=3)), (box, with_ids)
    # ... and the tick matters: the same three substeps begun one tick later differ
    a, b = PC.reference(DC.BOXES[0], 3, False), PC.reference(DC.BOXES[0], 3, False, tick=PC.TICK + 1)
    assert not DN.same(a[0], b[0])


def test_a_path_follows_the_id_not_the_slot():
    box, n = DC.BOXES[0], 20000
    px, py, st = (a[:n].copy() for a in DC.particles())
    ids = PC.ids()[:n].copy()
    PN.dispersal_step(DC.H, 2, PC.KH, PC.SEED, PC.TICK, box, *DC.flow(), px, py, st, ids)
    perm = np.random.default_rng(3).permutation(n)
    qx, qy, qs, qi = px[perm].copy(), py[perm].copy(), st[perm].copy(), ids[perm].copy()
    PN.dispersal_step(DC.H, 2, PC.KH, PC.SEED, PC.TICK + 2, box, *DC.flow(), qx, qy, qs, qi)
    want = PC.reference(box, 2, True, calls=2)
    back = np.empty(n, dtype=np.int64)
    back[perm] = np.arange(n)
    assert _same3((qx[back], qy[back], qs[back]), want, n)
    # without the ids carried the slots' numbers are the identities, and the permuted run is another run
    rx, ry, rs = px[perm].copy(), py[perm].copy(), st[perm].copy()
    PN.dispersal_step(DC.H, 2, PC.KH, PC.SEED, PC.TICK + 2, box, *DC.flow(), rx, ry, rs, ids)
    assert not DN.same(rx[back], want[0][:n])


def test_in_still_water_nobody_is_grounded():
    tm, dx_t, dy_t, un, vn = DC.flow()
    still = np.zeros_like(un)
    for box in DC.BOXES:
        px, py, st = (a.copy() for a in DC.particles())
        # the entry test grounds whoever was seeded on land: they are not the rule's doing
        DN.drifter_step(DC.H, 1, box, tm, dx_t, dy_t, still, still, px, py, st)
        x0, y0, s0 = px.copy(), py.copy(), st.copy()
        seen = {}
        for c in range(4):
            PN.dispersal_step(DC.H, 3, PC.KH, PC.SEED, 3 * c, box, tm, dx_t, dy_t, still, still, px, py, st, PC.ids(), seen)
        assert seen["grounded"] == 0 and seen["rejected"] > 1000, seen
        assert ((st == DN.GROUNDED) == (s0 == DN.GROUNDED)).all()
        assert ((st == DN.LEFT) & (s0 == DN.ACTIVE)).sum() > 100 and (st == DN.ACTIVE).sum() > 30000
        # a rejected kick leaves the particle where it was: whoever is still ACTIVE is on a wet cell
        act = st == DN.ACTIVE
        assert (tm[np.floor(py[act]).astype(int) - 1, np.floor(px[act]).astype(int) - 1] > 0).all()
        moved = act & ((px != x0) | (py != y0))
        assert moved.sum() > 30000


def test_the_case_takes_every_branch_of_the_kick():
    px, py, st, seen = PC.reference(DC.BOXES[0], 3, False)
    assert seen["rejected"] > 100 and seen["left_by_kick"] > 100 and seen["open_by_kick"] > 100, seen
    assert seen["grounded"] > 100 and (st == DN.GROUNDED).sum() > 100, seen
    assert all((st == s).sum() > 100 for s in range(4))
    scalar = PC.scalar_reference(DC.BOXES[0], 3, False)[3]
    assert all(scalar.get(k, 0) > 0 for k in ("rejected", "left_by_kick", "open_by_kick", "grounded")), scalar


def test_the_cloud_of_a_point_release_spreads_as_the_diffusivity_says():
    """still water, a uniform 1000 m mesh, every cell wet, a box that nobody can leave in 64 substeps of at most 0.3 cells;
    the bounds are five standard errors of a sample of n"""
    n, steps, size, mesh = 2 ** 16, 64, 48, 1000.0
    tm = np.ones((size, size), dtype=np.int32)
    d = np.full((size, size), mesh)
    still = np.zeros((size, size))
    box = (2, size - 1, 2, size - 1)
    px, py, st = np.full(n, 24.5), np.full(n, 24.5), np.zeros(n, dtype=np.int32)
    for c in range(steps // 16):
        PN.dispersal_step(DC.H, 16, PC.KH, PC.SEED, 16 * c, box, tm, d, d, still, still, px, py, st)
    assert (st == DN.ACTIVE).all()
    ex, ey = (px - 24.5) * mesh, (py - 24.5) * mesh
    var = 2.0 * PC.KH * (steps * DC.H)
    for e in (ex, ey):
        assert abs(e.var(ddof=1) / var - 1.0) < 5.0 * np.sqrt(2.0 / n), e.var(ddof=1) / var
        assert abs(e.mean()) < 5.0 * np.sqrt(var / n), e.mean()
    assert abs(np.corrcoef(ex, ey)[0, 1]) < 5.0 / np.sqrt(n)
    print("variance ratios %.5f %.5f (bound %.5f), means %.2f %.2f m (bound %.2f), correlation %.5f (bound %.5f)" % (
        ex.var(ddof=1) / var, ey.var(ddof=1) / var, 5.0 * np.sqrt(2.0 / n), ex.mean(), ey.mean(), 5.0 * np.sqrt(var / n),
        np.corrcoef(ex, ey)[0, 1], 5.0 / np.sqrt(n)))
