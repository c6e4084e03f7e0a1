"""CPU tests of the particle migration's rule through its two restatements in
tests/particle_migrate_numpy.py and the World built on them: the scalar and the array form agree; on five meshes every id is in
exactly one slot after every step; a corner crossing arrives within one call; a small cap holds and later delivers; too few
FREE slots are counted as dropped; a NaN and a LEFT particle at the edge of the global domain stay; and on the lattice flow the
World equals the undivided run bit for bit."""
import numpy as np
import pytest

import drifter_numpy as DN
import particle_migrate_numpy as M

BOX = (3, 40, 2, 21)


def random_set(n, seed, npayload, leaving=0.3, free=0.2):
    """slots around BOX: ACTIVE inside, LEFT on every side (corners, NaN and infinities among them), FREE, other statuses"""
    rng = np.random.default_rng(seed)
    xs, xe, ys, ye = BOX
    px = xs + (xe + 1 - xs) * rng.random(n)
    py = ys + (ye + 1 - ys) * rng.random(n)
    st = np.zeros(n, dtype=np.int32)
    out = rng.random(n) < leaving
    side = rng.integers(0, 8, n)
    px = np.where(out & np.isin(side, (0, 4, 5)), xs - 3 * rng.random(n) - 1e-9, px)
    px = np.where(out & np.isin(side, (1, 6, 7)), xe + 1 + 3 * rng.random(n), px)
    py = np.where(out & np.isin(side, (2, 4, 6)), ys - 3 * rng.random(n) - 1e-9, py)
    py = np.where(out & np.isin(side, (3, 5, 7)), ye + 1 + 3 * rng.random(n), py)
    st[out] = M.LEFT
    odd = rng.random(n)
    px[out & (odd < 0.02)] = np.nan
    py[out & (odd > 0.98)] = np.inf
    px[out & (odd > 0.96) & (odd <= 0.98)] = -np.inf
    st[~out & (rng.random(n) < free)] = M.FREE
    st[~out & (st == 0) & (rng.random(n) < 0.05)] = M.GROUNDED
    st[~out & (st == 0) & (rng.random(n) < 0.05)] = M.LEFT          # LEFT but inside the box: stays
    ids = rng.integers(-2 ** 62, 2 ** 62, n)
    payload = [rng.integers(-2 ** 62, 2 ** 62, n) if q % 2 == 0 else rng.random(n) for q in range(npayload)]
    return px, py, st, ids, payload


def run_pair(fn_pack, fn_unpack, axis, data, has, cap, recv_of=None):
    px, py, st, ids, payload = (a.copy() if not isinstance(a, list) else [b.copy() for b in a] for a in data)
    npay = len(payload)
    send = [M.new_message(cap, npay) for _ in range(2)]
    counts = np.full(M.RECORD, -9, dtype=np.int32)
    if axis == M.AXIS_Y:
        counts[M.DROPPED], counts[M.BAD] = 2, 0
    fn_pack(axis, BOX, px, py, st, ids, payload, has, (38, -38), (5, -7), cap, send, counts)
    recv = [send[1].copy(), send[0].copy()] if recv_of is None else recv_of
    fn_unpack(axis, BOX, px, py, st, ids, payload, cap, recv, counts)
    return px, py, st, ids, payload, send, counts


def same_result(a, b):
    for x, y in zip(a[:4], b[:4]):
        assert DN.same(x, y)
    for x, y in zip(a[4], b[4]):
        assert DN.same(x, y)
    for x, y in zip(a[5], b[5]):
        assert (x == y).all()
    assert (a[6] == b[6]).all(), (a[6], b[6])


@pytest.mark.parametrize("axis", [M.AXIS_X, M.AXIS_Y])
@pytest.mark.parametrize("npayload", [0, 4])
def test_the_two_forms_agree(axis, npayload):
    for n, cap, has in ((0, 1, (1, 1)), (1, 1, (1, 1)), (65, 3, (1, 1)), (300, 300, (1, 0)), (300, 7, (0, 1)), (2000, 32, (1, 1)),
                        (2000, 2000, (0, 0))):
        data = random_set(n, 100 + n + cap, npayload)
        a = run_pair(M.pack_scalar, M.unpack_scalar, axis, data, has, cap)
        b = run_pair(M.pack_vector, M.unpack_vector, axis, data, has, cap)
        same_result(a, b)
        sent, held = a[6][2 * axis:2 * axis + 2], a[6][4 + 2 * axis:6 + 2 * axis]
        assert (sent <= cap).all() and (held >= 0).all()
        if n == 2000 and cap == 32:
            assert (sent == 32).all() and (held > 0).all()          # the case holds particles
        if not any(has):
            assert (sent == 0).all() and (held == 0).all() and DN.same(a[0], data[0]) and (a[2] == data[2]).all()
        # what was not sent is untouched, and the words past count keep the sentinel
        for d in range(2):
            c = int(a[5][d][0])
            for w in range(3 + npayload):
                assert (M.field(a[5][d], cap, w)[c:] == M.SENTINEL).all()
            assert a[5][d][1] == M.SENTINEL


def test_a_bad_header_unpacks_nothing():
    data = random_set(500, 5, 1)
    for bad, bit in ((-1, 1), (9, 2)):
        recv = [M.empty_message(8, 1), M.empty_message(8, 1)]
        recv[bit - 1][:1] = np.array([bad], dtype=np.int64).view(np.uint64)
        for fns in ((M.pack_scalar, M.unpack_scalar), (M.pack_vector, M.unpack_vector)):
            got = run_pair(*fns, M.AXIS_X, data, (0, 0), 8, recv_of=recv)
            assert got[6][M.BAD] == bit and got[6][M.DROPPED] == 0 and (got[6][8:10] == 0).all()
            assert DN.same(got[0], data[0]) and (got[2] == data[2]).all()


MESHES = [(1, 2), (2, 1), (2, 2), (3, 2), (1, 4)]


@pytest.mark.parametrize("mesh", MESHES, ids=lambda m: "%dx%d" % m)
def test_every_id_is_in_exactly_one_slot_after_every_step(mesh):
    nx, ny, steps = 48, 40, 30
    flow = M.gyre(nx, ny)
    rng = np.random.default_rng(7)
    x, y = 2.0 + nx * rng.random(3000), 2.0 + ny * rng.random(3000)
    w = M.World(flow, M.make_tiles(nx, ny, *mesh), mesh, nslots=4096, cap=5, x=x, y=y, npayload=2)
    moved = 0
    for _ in range(steps):
        w.step(400.0)
        seen = w.census()
        assert sorted(seen) == list(range(3000))
        for c in w.counts:
            assert c[M.DROPPED] == 0 and c[M.BAD] == 0
            moved += int(c[0:4].sum())
        for r in range(len(w.tiles)):                               # the payload has travelled with its id
            live = w.st[r] != M.FREE
            assert (w.payload[r][0][live] == w.ids[r][live] * 3).all()
            assert (w.payload[r][1][live] == w.ids[r][live] * 0.5 + 1).all()
    assert moved > 100 and w.held > 0                               # particles crossed, and cap = 5 held some back


def test_a_corner_crossing_arrives_within_one_call():
    nx, ny = 16, 12
    flow, _ = M.lattice(nx, ny)
    flow = (np.ones_like(flow[0]),) + flow[1:]                      # no island
    tiles = M.make_tiles(nx, ny, 2, 2)                              # tile 0: global columns 2..9, rows 2..7
    x, y = np.array([9.875, 9.875, 5.0]), np.array([7.9375, 5.0, 7.9375])
    w = M.World(flow, tiles, (2, 2), nslots=8, cap=4, x=x, y=y)
    w.step(250.0)
    seen = w.census()
    assert seen[0] == (M.ACTIVE, 10.125, 8.0625)
    where = {int(i): r for r in range(4) for i in w.ids[r][w.st[r] != M.FREE]}
    assert where == {0: 3, 1: 1, 2: 2}
    assert list(w.counts[0][0:4]) == [0, 2, 0, 1]                   # tile 0 sent two E and one N
    assert list(w.counts[1][8:12]) == [2, 0, 0, 0] and list(w.counts[1][0:4]) == [0, 0, 0, 1]      # tile 1 forwarded one N
    assert list(w.counts[3][8:12]) == [0, 0, 1, 0]


def test_cap_one_holds_and_later_delivers():
    nx, ny = 16, 12
    flow, _ = M.lattice(nx, ny)
    flow = (np.ones_like(flow[0]),) + flow[1:]
    x, y = np.full(5, 9.875), 3.0 + np.arange(5.0)
    w = M.World(flow, M.make_tiles(nx, ny, 2, 1), (2, 1), nslots=8, cap=1, x=x, y=y)
    w.advect(250.0)
    for call in range(5):
        w.migrate()
        assert w.counts[0][M.E] == 1 and w.counts[0][4 + M.E] == 4 - call
        there = sorted(int(i) for i in w.ids[1][w.st[1] != M.FREE])
        assert there == list(range(call + 1))                        # the lowest slot goes first
        assert int(np.count_nonzero(w.st[0] == M.LEFT)) == 4 - call
    assert sorted(w.census()) == list(range(5))


def test_too_few_free_slots_are_counted_as_dropped():
    nx, ny = 16, 12
    flow, _ = M.lattice(nx, ny)
    flow = (np.ones_like(flow[0]),) + flow[1:]
    x = np.concatenate([np.full(4, 9.875), 10.5 + np.arange(6.0)])
    y = np.concatenate([3.0 + np.arange(4.0), np.full(6, 4.5)])
    w = M.World(flow, M.make_tiles(nx, ny, 2, 1), (2, 1), nslots=7, cap=8, x=x, y=y)       # tile 1: six of seven slots taken
    w.step(250.0)
    assert w.counts[0][M.E] == 4 and w.counts[1][8 + M.W] == 1 and w.counts[1][M.DROPPED] == 3 and w.counts[1][M.NFREE] == 0
    assert w.counts[0][M.NFREE] == 7


def test_a_nan_and_a_left_at_the_global_edge_stay():
    nx, ny = 16, 12
    flow, _ = M.lattice(nx, ny)
    flow = (np.ones_like(flow[0]),) + flow[1:]
    tiles = M.make_tiles(nx, ny, 2, 2)
    x, y = np.array([17.9, 12.0, 17.9, 4.0]), np.array([4.0, 13.95, 7.95, 4.0])
    w = M.World(flow, tiles, (2, 2), nslots=6, cap=4, x=x, y=y)
    w.px[0][w.ids[0] == 3] = np.nan                                  # becomes LEFT at a NaN
    w.step(250.0)
    seen = w.census()
    assert seen[0][0] == M.LEFT and seen[0][1] == 18.15              # east of the global domain: no neighbour
    assert seen[1][0] == M.LEFT and seen[1][2] > 14.0                # north of it
    # id 2 left tile 1 east (no neighbour) and north (a neighbour): it stays where it is, in tile 1
    assert seen[2][0] == M.LEFT and 2 in w.ids[1][w.st[1] == M.LEFT]
    assert seen[3][0] == M.LEFT and np.isnan(seen[3][1]) and 3 in w.ids[0]
    for c in w.counts:
        assert (c[0:12] == 0).all() and c[M.DROPPED] == 0
    before = [(a.copy(), b.copy(), c.copy()) for a, b, c in zip(w.px, w.py, w.st)]
    w.migrate()
    for r in range(4):
        assert DN.same(before[r][0], w.px[r]) and DN.same(before[r][1], w.py[r]) and (before[r][2] == w.st[r]).all()


@pytest.mark.parametrize("mesh", [(2, 2), (3, 2)], ids=lambda m: "%dx%d" % m)
def test_lattice_flow_equals_the_undivided_run_bit_for_bit(mesh):
    """un = 1, vn = 0.5, dx = dy = 1000, h = 250, nsub = 1: a step moves (1/4, 1/8), start positions are multiples of 1/8,
    every position a multiple of 1/16 far below 2^53, so a shift by whole cells is exact and the frames agree"""
    nx, ny, steps = 48, 40, 44
    flow, isl = M.lattice(nx, ny)
    x, y = M.lattice_seeds(nx, ny, isl, steps)
    n = len(x)
    assert n > 1500
    gx, gy, gst = x.copy(), y.copy(), np.zeros(n, dtype=np.int32)
    w = M.World(flow, M.make_tiles(nx, ny, *mesh), mesh, nslots=2048, cap=64, x=x, y=y)
    crossed = corner = 0
    for step in range(steps):
        DN.drifter_step(250.0, 1, (2, nx + 1, 2, ny + 1), *flow, gx, gy, gst)
        w.step(250.0)
        seen = w.census()
        assert sorted(seen) == list(range(n))
        st = np.array([seen[i][0] for i in range(n)])
        sx, sy = np.array([seen[i][1] for i in range(n)]), np.array([seen[i][2] for i in range(n)])
        assert (st == gst).all(), step
        assert DN.same(sx, gx) and DN.same(sy, gy), step
        assert ((gx * 16) % 1 == 0).all() and ((gy * 16) % 1 == 0).all()
        crossed += sum(int(c[0:4].sum()) for c in w.counts)
        corner += sum(int(c[2:4].sum() > 0 and c[8:10].sum() > 0) for c in w.counts)
    assert crossed > 300 and corner > 0
    assert (gst == DN.GROUNDED).sum() > 10 and (gst == DN.LEFT).sum() > 10 and (gst == DN.ACTIVE).sum() > 100
