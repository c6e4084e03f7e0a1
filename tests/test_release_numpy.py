"""CPU tests of the release rule as tests/release_numpy.py restates it twice: the two restatements
agree to the bit on every shared case (tests/release_cases.py), the record's invariant holds, the rounding edge yields one LEFT
particle, a release in two calls is the release in one, the tiles of a 2 x 2 and a 3 x 2 decomposition release between them
exactly the wet in-domain particles of the undivided run, a patch is uniform to five standard errors, and nothing is released
onto land."""
import numpy as np
import pytest

import particle_migrate_numpy as M
import release_cases as RC
import release_numpy as R

CASES = RC.cases()


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_the_two_restatements_agree_to_the_bit_and_the_invariant_holds():
    seen = np.zeros(R.RECORD, dtype=np.int64)
    for c in CASES + [RC.deep_slots_case()]:
        va, vs, vr = RC.reference(c) if c["n"] < 10 ** 6 else RC.run(c)
        sa, ss, sr = RC.run(c, R.release_scalar)
        assert all(_same(a, b) for a, b in zip(va, sa)), c["name"]
        assert _same(vs, ss) and _same(vr, sr), (c["name"], vr, sr)
        assert R.invariant(vr) and (vr[10:] == 0).all(), (c["name"], vr)
        assert vr[R.NFREE] == np.count_nonzero(va[2] == R.FREE), c["name"]
        seen += vr != 0
        # every word the rule does not name keeps its sentinel
        start = RC.arrays(c)
        new = start[2] != va[2]
        assert np.count_nonzero(new) == vr[R.RELEASED] and (start[2][new] == R.FREE).all(), c["name"]
        for k in (0, 1):
            assert (va[k][~new] == RC.SENT_F).all(), c["name"]
        for k in (3, 4, 5):
            assert va[k] is None or (va[k][~new] == RC.SENT_I).all(), c["name"]
        if va[5] is not None:
            assert (va[5][new] == RC.TICK + RC.TICK_DEV).all(), c["name"]
    # between them the cases reach every word of the record
    assert (seen[[0, 2, 3, 4, 5, 6, 7, 8, 9]] > 0).all(), seen


def test_the_rounding_edge_yields_one_left_particle():
    c = next(c for c in CASES if c["name"] == "edge")
    arr, src, rec = RC.reference(c)
    assert rec[R.EDGE] == 1 and rec[R.RELEASED] == 1 and R.requested(rec) == 1
    assert arr[2][0] == R.LEFT and arr[0][0] == 18.0 and arr[3][0] == 7 and src[0, R.NEXT_ID] == 8


def test_sources_that_do_not_count():
    c = RC.case("counts", n=12289, pattern="all", max_count=256, src=RC.sources((0, 0), shift=3))
    arr, src, rec = RC.run(c)
    assert rec[R.BAD_SOURCE] == 5 and (src[6:11, R.NEXT_ID] == c["sources"][6:11, R.NEXT_ID]).all()
    assert rec[R.CLAMPED] == np.count_nonzero(c["sources"][:, R.COUNT] > c["max_count"]) > 0
    given = src[:, R.NEXT_ID].astype(np.uint64) - c["sources"][:, R.NEXT_ID].astype(np.uint64)
    assert given.sum() == R.requested(rec) and given.max() == c["max_count"]
    assert src[4, R.NEXT_ID] < 0 < c["sources"][4, R.NEXT_ID]                                  # wrapped
    assert (np.delete(src, R.NEXT_ID, axis=1) == np.delete(c["sources"], R.NEXT_ID, axis=1)).all()


@pytest.mark.parametrize("how", [R.release_scalar, R.release_vector])
def test_two_calls_continue_the_ids(how):
    """releasing a then b gives the (id, position) set of a + b at once"""
    a, b = 100, 156
    c = RC.case("split", off=RC.OFFSETS[1], n=12289, pattern="all", max_count=256,
                src=RC.sources(RC.OFFSETS[1], counts=[a + b]))
    whole, wsrc, wrec = RC.run(c, how)
    parts = RC.arrays(c)
    src = c["sources"].copy()
    for k in (a, b):
        src[:, R.COUNT] = np.where(src[:, R.COUNT] >= 0, k, -1)
        _, src, rec = RC.run(c, how, arr=parts, src=src)
        assert R.invariant(rec)
    assert (src[:, R.NEXT_ID] == wsrc[:, R.NEXT_ID]).all()
    assert RC.census(parts, c["off"]) == RC.census(whole, c["off"]) and len(RC.census(whole, c["off"])) > 500


@pytest.mark.parametrize("mesh", [(2, 2), (3, 2)])
def test_the_tiles_release_the_undivided_run(mesh):
    tm = RC.basin_mask()
    count = 300
    src = RC.basin_sources(count)
    one = M.make_tiles(*RC.BASIN, 1, 1)[0]
    arr, after, rec = RC.run(RC.tile_case(one, src, count), tm=M.window(tm, one))
    want = RC.census(arr, one["off"])
    assert rec[R.DROPPED] == 0 and rec[R.FOREIGN] > 0 and rec[R.ON_LAND] > 0 and len(want) == rec[R.RELEASED] > 1000
    got, foreign = {}, 0
    for t in M.make_tiles(*RC.BASIN, *mesh):
        tarr, tafter, trec = RC.run(RC.tile_case(t, src, count), tm=M.window(tm, t))
        assert (tafter == after).all() and trec[R.DROPPED] == 0 and R.invariant(trec)
        mine = RC.census(tarr, t["off"])
        assert not set(mine) & set(got), "a particle was released on two tiles"
        got.update(mine)
        foreign += trec[R.FOREIGN]
    assert got == want
    # every candidate is foreign on all tiles but its owner's, and on all if it lies outside the domain
    ntiles = mesh[0] * mesh[1]
    assert foreign == (ntiles - 1) * (R.requested(rec) - rec[R.FOREIGN]) + ntiles * rec[R.FOREIGN]


def test_a_patch_is_uniform_and_nothing_lands_on_land():
    n, rx, ry, x, y = 40000, 3.0, 2.0, 20.25, 17.5
    tm = np.ones((40, 44), dtype=np.int32)
    c = dict(name="uniform", box=(2, 43, 2, 39), off=(0, 0), n=n, pattern="all", max_count=n,
             sources=R.table([x], [y], [rx], [ry], [2 ** 40], [n]), optional=False, seed=RC.SEED)
    arr, _, rec = RC.run(c, tm=tm)
    assert rec[R.RELEASED] == n and (arr[2] == R.ACTIVE).all()
    for v, centre, r in ((arr[0], x, rx), (arr[1], y, ry)):
        assert abs(v.mean() - centre) <= 5 * np.sqrt(r * r / 3 / n)
        assert abs(v.var() - r * r / 3) <= 5 * np.sqrt(4 * r ** 4 / 45 / n)
        assert v.min() > centre - r and v.max() < centre + r
    assert abs(np.corrcoef(arr[0], arr[1])[0, 1]) <= 5 / np.sqrt(n)
    # no particle of any case stands on land
    tm = RC.mask()
    for c in CASES:
        px, py, st = RC.reference(c)[0][:3]
        live = st == R.ACTIVE
        assert (tm[np.floor(py[live]).astype(int) - 1, np.floor(px[live]).astype(int) - 1] != 0).all(), c["name"]
        assert np.isin(st, (R.ACTIVE, R.LEFT, R.FREE, RC.SENT_ST)).all()
