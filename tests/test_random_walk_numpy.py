"""CPU tests of the random walk in a varying diffusivity as tests/random_walk_numpy.py restates it:
the scalar and the array restatement agree bit for bit, census included, on the shared field and on one that breaks the
contract; a constant field gives dispersal_numpy's bits and a zero field drifter_numpy's; what kh_t holds on land changes no
bit; one call with nsub = k is k calls at successive ticks; a path follows the id, not the slot; in still water nobody is
GROUNDED; the shared case takes every branch; and in a closed basin a uniform cloud stays uniform within five multinomial
standard errors, while the same walk without the drift does not."""
import numpy as np

import dispersal_cases as PC
import drifter_cases as DC
import drifter_numpy as DN
import random_walk_cases as RC
import random_walk_numpy as RN


def _same3(a, b, n=None):
    return DN.same(a[0][:n], b[0][:n]) and DN.same(a[1][:n], b[1][:n]) and bool((a[2][:n] == b[2][:n]).all())


def test_the_two_restatements_agree():
    cases = [(box, nsub, with_ids, "kh") for box in DC.BOXES for nsub in (1, 3) for with_ids in (False, True)]
    cases.append((DC.BOXES[0], 3, True, "bad"))
    for box, nsub, with_ids, field in cases:
        a, s = RC.reference(box, nsub, with_ids, field), RC.scalar_reference(box, nsub, with_ids, field)
        assert _same3(a, s, DC.NSCALAR), (box, nsub, with_ids, field)
        # the census of the array form over the scalar form's particles is the scalar form's
        px, py, st = (v[:DC.NSCALAR].copy() for v in DC.particles())
        seen = {}
        kh = RC.kh_field() if field == "kh" else RC.bad_field()
        RN.random_walk(DC.H, nsub, kh, RC.SEED, RC.TICK, box, *DC.flow(), px, py, st,
                       RC.ids()[:DC.NSCALAR] if with_ids else None, seen)
        assert {k: v for k, v in seen.items() if v} == s[3], (box, nsub, with_ids, field)
    a, b = RC.reference(DC.BOXES[0], 3, False), RC.reference(DC.BOXES[0], 3, True)
    assert not DN.same(a[0], b[0])                                              # the ids matter
    assert not DN.same(a[0], PC.reference(DC.BOXES[0], 3, False)[0])            # ... and so does the field
    assert not DN.same(a[0], RC.reference(DC.BOXES[0], 3, False, "bad")[0])
    idle = DC.particles()[2] != DN.ACTIVE
    assert DN.same(a[0][idle], DC.particles()[0][idle]) and (a[2][idle] == DC.particles()[2][idle]).all()


def test_a_constant_field_is_the_dispersal_step_and_a_zero_field_the_drifter_step():
    for box in DC.BOXES:
        for nsub in (1, 3):
            for with_ids in (False, True):
                got = RC.reference(box, nsub, with_ids, PC.KH)
                assert _same3(got, PC.reference(box, nsub, with_ids)), (box, nsub, with_ids)
            assert _same3(RC.scalar_reference(box, nsub, True, PC.KH), PC.scalar_reference(box, nsub, True)), (box, nsub)
            zero = RC.reference(box, nsub, True, 0.0)
            assert _same3(zero, DC.reference(box, nsub)), (box, nsub)
            assert _same3(RC.scalar_reference(box, nsub, False, 0.0), DC.scalar_reference(box, nsub)), (box, nsub)


def test_what_the_field_holds_on_land_changes_no_bit():
    box = DC.BOXES[0]
    rng = np.random.default_rng(5)
    for fill in (0.0, -5.0, np.inf, None):
        kh = RC.kh_field().copy()
        land = DC.mask() == 0
        kh[land] = 1e6 * rng.random(int(land.sum())) if fill is None else fill
        px, py, st = (a.copy() for a in DC.particles())
        RN.random_walk(DC.H, 3, kh, RC.SEED, RC.TICK, box, *DC.flow(), px, py, st, RC.ids())
        assert _same3((px, py, st), RC.reference(box, 3, True)), fill


def test_one_call_with_nsub_k_is_k_calls_at_successive_ticks():
    for box in DC.BOXES:
        for with_ids in (False, True):
            assert _same3(RC.reference(box, 3, with_ids), RC.reference(box, 1, with_ids, calls=3)), (box, with_ids)
    a, b = RC.reference(DC.BOXES[0], 3, False), RC.reference(DC.BOXES[0], 3, False, tick=RC.TICK + 1)
    assert not DN.same(a[0], b[0])


def test_a_path_follows_the_id_not_the_slot():
    box, n, kh = DC.BOXES[0], 20000, RC.kh_field()
    px, py, st = (a[:n].copy() for a in DC.particles())
    ids = RC.ids()[:n].copy()
    RN.random_walk(DC.H, 2, kh, RC.SEED, RC.TICK, box, *DC.flow(), px, py, st, ids)
    perm = np.random.default_rng(3).permutation(n)
    qx, qy, qs, qi = px[perm].copy(), py[perm].copy(), st[perm].copy(), ids[perm].copy()
    RN.random_walk(DC.H, 2, kh, RC.SEED, RC.TICK + 2, box, *DC.flow(), qx, qy, qs, qi)
    want = RC.reference(box, 2, True, calls=2)
    back = np.empty(n, dtype=np.int64)
    back[perm] = np.arange(n)
    assert _same3((qx[back], qy[back], qs[back]), want, n)
    rx, ry, rs = px[perm].copy(), py[perm].copy(), st[perm].copy()
    RN.random_walk(DC.H, 2, kh, RC.SEED, RC.TICK + 2, box, *DC.flow(), rx, ry, rs, ids)
    assert not DN.same(rx[back], want[0][:n])


def test_in_still_water_nobody_is_grounded():
    tm, dx_t, dy_t, un, vn = DC.flow()
    still = np.zeros_like(un)
    for box in DC.BOXES:
        px, py, st = (a.copy() for a in DC.particles())
        DN.drifter_step(DC.H, 1, box, tm, dx_t, dy_t, still, still, px, py, st)      # the entry test's GROUNDED are not the rule's
        s0 = st.copy()
        seen = {}
        for c in range(4):
            RN.random_walk(DC.H, 3, RC.kh_field(), RC.SEED, 3 * c, box, tm, dx_t, dy_t, still, still, px, py, st, RC.ids(), seen)
        assert seen["grounded"] == 0 and seen["rejected"] > 1000, seen
        assert ((st == DN.GROUNDED) == (s0 == DN.GROUNDED)).all()
        act = st == DN.ACTIVE
        assert act.sum() > 30000 and (tm[np.floor(py[act]).astype(int) - 1, np.floor(px[act]).astype(int) - 1] > 0).all()


def test_the_case_takes_every_branch():
    """a condition of the shared case: every member of the census is above zero, for either restatement alone"""
    px, py, st, seen = RC.reference(DC.BOXES[0], 3, False)
    print(seen)
    assert set(seen) == set(RN.CENSUS) and all(v > 100 for v in seen.values()), seen
    assert all((st == s).sum() > 100 for s in range(4))
    scalar = RC.scalar_reference(DC.BOXES[0], 3, False)[3]
    print(scalar)
    assert all(scalar.get(k, 0) > 0 for k in RN.CENSUS), scalar
    # the zeros and the steep part are where the particles are: K = 0 on both faces clamps, and a face difference of 74 m2/s
    # in a cell drifts a particle by a few hundredths of a cell
    kh, tm = RC.kh_field(), DC.mask()
    assert (kh[tm != 0] >= 0.0).all() and np.isnan(kh[tm == 0]).all() and (kh[tm > 0] == 0.0).sum() == 11
    assert np.nanmax(np.abs(np.diff(kh[:, 17:21], axis=1))) == 148.0
    # with values >= 0 the clamp is never reached from below: the field that breaks the contract does reach it more often
    assert RC.reference(DC.BOXES[0], 3, False, "bad")[3]["clamped"] > seen["clamped"]


def test_a_well_mixed_cloud_stays_well_mixed():
    """2^14 particles uniform over a closed 16 x 16 basin of 1000 m cells in still water, K = 50 (1 + 0.9 sin)(1 + 0.9 sin)
    m2/s, h = 400 s, 800 substeps.  Every column and every row count lies within 5 multinomial standard errors of N / 16;
    the same walk without the drift and with the own cell's K (the scheme this rule replaces) is beyond 20 in some bin.
    On the CPU: 2.4 and 3.1 with the drift, 46 and 39 without."""
    box, tm, dx, dy, un, vn, kh = RC.basin()
    worst = {}
    for naive in (False, True):
        px, py, st = RC.basin_release()
        for c in range(RC.WM_STEPS // RC.WM_SUB):
            RN.random_walk(RC.WM_H, RC.WM_SUB, kh, RC.SEED, c * RC.WM_SUB, box, tm, dx, dy, un, vn, px, py, st, naive=naive)
        worst[naive] = RC.marginal_errors(px, py, st)
    print("largest deviation of a column and of a row count, in standard errors: %.2f %.2f with the drift, %.1f %.1f without"
          % (worst[False] + worst[True]))
    assert max(worst[False]) < 5.0, worst
    assert max(worst[True]) > 20.0, worst
