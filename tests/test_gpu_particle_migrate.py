"""GPU tests (-m gpu) of the particle migration in one process: dlesm_migrate_pack_f64 and
dlesm_migrate_unpack_f64 against the array restatement (tests/particle_migrate_numpy.py) bit for bit -- the particle arrays,
every word of the sentinel-filled messages, the record, and guard bytes behind the scratch -- over eleven counts, the two
counts just past the sizes at which the pack's and the unpack's scan take their multi-block path, seven distributions, four
caps, both payload counts and both axes; a bad header count; a World of 2 x 2 and 3 x 2 sub-boxes of one gyre stepped by
the real dlesm_drifter_step_f64 with the messages routed by torch copies, against the numpy World after every step; the
lattice flow against the undivided device run; one rank as its own W and E neighbour through dlesm_migrate_f64; pack and
unpack captured into a graph and replayed on changing data, and on two streams; the Python wrapper.  Everything is an integer
or a bit pattern: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import drifter_numpy as DN
import particle_migrate_numpy as M

pytestmark = pytest.mark.gpu
GUARD = 256
SLACK, SLOT_FILL = 8, -9          # guard elements behind every particle array
BYTE_FILL = 0xA5
BOX = (3, 40, 2, 21)
NS = [0, 1, 63, 64, 65, 255, 256, 257, 4096, 4097, 70001]
DISTS = ["nobody", "one_side", "alternating", "all_free", "no_free", "last_wave", "specials"]


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    import dl_esm_inf_amd as d
    torch.cuda.set_device(0)
    d.parallel_init(0, 1)
    yield torch, d, d._cabi.lib()


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _sp(stream):
    return C.c_void_p(stream.cuda_stream) if stream is not None else None


def _i2(v):
    return (C.c_int * len(v))(*[int(a) for a in v])


def _pp(tensors):
    return (C.c_void_p * max(len(tensors), 1))(*[t.data_ptr() for t in tensors])


def make_set(dist, n, axis, npayload, seed):
    """(px, py, status, ids, payload) on the host around BOX"""
    rng = np.random.default_rng(seed)
    xs, xe, ys, ye = BOX
    px = xs + (xe + 1 - xs) * rng.random(n)
    py = ys + (ye + 1 - ys) * rng.random(n)
    st = np.zeros(n, dtype=np.int32)
    lo = (xs - 1.5, None) if axis == M.AXIS_X else (None, ys - 1.5)
    hi = (xe + 2.5, None) if axis == M.AXIS_X else (None, ye + 2.5)

    def leave(mask, where):
        if where[0] is not None:
            px[mask] = where[0]
        else:
            py[mask] = where[1]
        st[mask] = M.LEFT

    k = np.arange(n)
    if dist == "one_side":
        leave(k >= 0, lo)
    elif dist == "alternating":
        leave(k % 2 == 0, lo), leave(k % 2 == 1, hi)
    elif dist == "all_free":
        st[:] = M.FREE
    elif dist == "no_free":
        leave(rng.random(n) < 0.3, hi), leave(rng.random(n) < 0.1, lo)
    elif dist == "last_wave":
        leave(k >= max(0, n - 1 - (n - 1) % 64), hi)
    elif dist == "specials":
        out = rng.random(n) < 0.4
        side = rng.integers(0, 8, n)
        px = np.where(out & np.isin(side, (0, 4, 5)), xs - 3 * rng.random(n) - 1e-9, px)
        px = np.where(out & np.isin(side, (1, 6, 7)), xe + 1 + 3 * rng.random(n), px)
        py = np.where(out & np.isin(side, (2, 4, 6)), ys - 3 * rng.random(n) - 1e-9, py)
        py = np.where(out & np.isin(side, (3, 5, 7)), ye + 1 + 3 * rng.random(n), py)
        st[out] = M.LEFT
        odd = rng.random(n)
        px[out & (odd < 0.03)] = np.nan
        py[out & (odd > 0.97)] = np.inf
        px[out & (odd > 0.94) & (odd <= 0.97)] = -np.inf
        py[out & (odd > 0.91) & (odd <= 0.94)] = np.nan
        st[~out & (rng.random(n) < 0.25)] = M.FREE
        st[~out & (st == 0) & (rng.random(n) < 0.1)] = rng.integers(1, 9)
    ids = rng.integers(-2 ** 62, 2 ** 62, n)
    payload = [rng.integers(-2 ** 62, 2 ** 62, n) if q % 2 == 0 else rng.random(n) for q in range(npayload)]
    return px, py, st, ids, payload


def make_recv(cap, npayload, seed, counts=None):
    """two messages as a neighbour would have left them: a count, records around BOX, the sentinel behind them"""
    rng = np.random.default_rng(seed)
    out = []
    for d in range(2):
        m = M.new_message(cap, npayload)
        c = int(rng.integers(0, cap + 1)) if counts is None else counts[d]
        m[:1] = np.array([c], dtype=np.int64).view(np.uint64)
        c = max(0, min(c, cap))
        M.field(m, cap, 0)[:c] = (BOX[0] - 2 + (BOX[1] - BOX[0] + 5) * rng.random(c)).view(np.uint64)
        M.field(m, cap, 1)[:c] = (BOX[2] - 2 + (BOX[3] - BOX[2] + 5) * rng.random(c)).view(np.uint64)
        for w in range(2, 3 + npayload):
            M.field(m, cap, w)[:c] = rng.integers(0, 2 ** 63, c).astype(np.uint64)
        out.append(m)
    return out


class Dev:
    """a host set on the device, with its messages, record and scratch (GUARD guard bytes behind the stated size)"""

    def __init__(self, torch, L, host, cap, recv, counts):
        px, py, st, ids, payload = host
        self.n, self.cap, self.k = len(px), cap, len(payload)
        up = lambda a: torch.from_numpy(np.array(a)).cuda()

        def slots(a):                                                # SLACK guard elements behind the n slots
            return up(np.concatenate([a, np.full(SLACK, SLOT_FILL).astype(a.dtype)]))
        self.px, self.py, self.st, self.ids = slots(px), slots(py), slots(st), slots(ids)
        self.payload = [slots(a) for a in payload]
        self.send = [up(M.new_message(cap, self.k).view(np.int64)) for _ in range(2)]
        self.recv = [up(m.view(np.int64)) for m in recv]
        self.counts = up(counts)
        b = C.c_longlong(-1)
        assert L.dlesm_migrate_scratch(self.n, C.byref(b)) == 0 and b.value > 0
        self.need = b.value
        self.scratch = torch.full((self.need + GUARD,), BYTE_FILL, dtype=torch.uint8, device="cuda")
        b2 = C.c_longlong(-1)
        assert L.dlesm_migrate_bytes(cap, self.k, C.byref(b2)) == 0 and b2.value == 8 * M.message_words(cap, self.k)

    def pack(self, L, axis, has, sx, sy, stream=None, box=BOX):
        return L.dlesm_migrate_pack_f64(axis, *box, self.n, _ptr(self.px), _ptr(self.py), _ptr(self.st), _ptr(self.ids),
                                        _pp(self.payload), self.k, _i2(has), _i2(sx), _i2(sy), self.cap, _pp(self.send),
                                        _ptr(self.counts), _ptr(self.scratch), self.need, _sp(stream))

    def unpack(self, L, axis, stream=None, box=BOX, recv=None):
        return L.dlesm_migrate_unpack_f64(axis, *box, self.n, _ptr(self.px), _ptr(self.py), _ptr(self.st), _ptr(self.ids),
                                          _pp(self.payload), self.k, self.cap, _pp(recv or self.recv), _ptr(self.counts),
                                          _ptr(self.scratch), self.need, _sp(stream))

    def equals(self, want, send, counts):
        """None, or what differs from the host arrays"""
        px, py, st, ids, payload = want
        n = self.n
        got = [t.cpu().numpy() for t in [self.px, self.py, self.st, self.ids] + self.payload]
        for name, g, a in zip(["px", "py", "status", "id"] + ["payload %d" % q for q in range(self.k)], got,
                              [px, py, st, ids] + list(payload)):
            if not (g[n:] == np.full(SLACK, SLOT_FILL).astype(g.dtype)).all():
                return "the guard behind " + name
            if not (DN.same(g[:n], a) if g.dtype == np.float64 else (g[:n] == a).all()):
                return name
        for d in range(2):
            if send is not None and not (self.send[d].cpu().numpy().view(np.uint64) == send[d]).all():
                return "send %d" % d
        if not (self.counts.cpu().numpy() == counts).all():
            return "counts %s != %s" % (self.counts.cpu().numpy(), counts)
        if not bool((self.scratch[self.need:] == BYTE_FILL).all()):
            return "the guard behind the scratch"
        return None


def first_counts(axis):
    c = np.full(M.RECORD, -9, dtype=np.int32)
    if axis == M.AXIS_Y:
        c[M.DROPPED], c[M.BAD] = 2, 0
    return c


def pack_unpack_case(torch, L, dist, n, cap, npayload, axis, has, seed):
    host = make_set(dist, n, axis, npayload, seed)
    recv = make_recv(cap, npayload, seed + 1)
    dev = Dev(torch, L, host, cap, recv, first_counts(axis))
    sx, sy = (38, -38), (5, -7)
    assert dev.pack(L, axis, has, sx, sy) == 0, L.dlesm_last_error()
    want = [a.copy() for a in host[:4]] + [[a.copy() for a in host[4]]]
    send = [M.new_message(cap, npayload) for _ in range(2)]
    counts = first_counts(axis)
    M.pack_vector(axis, BOX, *want, has, sx, sy, cap, send, counts)
    torch.cuda.synchronize()
    bad = dev.equals(want, send, counts)
    assert bad is None, ("pack", bad, dist, n, cap, npayload, axis, has)
    assert dev.unpack(L, axis) == 0, L.dlesm_last_error()
    M.unpack_vector(axis, BOX, *want, cap, recv, counts)
    torch.cuda.synchronize()
    bad = dev.equals(want, send, counts)
    assert bad is None, ("unpack", bad, dist, n, cap, npayload, axis, has)
    for d in range(2):                                               # the messages read are unchanged
        assert (dev.recv[d].cpu().numpy().view(np.uint64) == recv[d]).all()
    return counts


@pytest.mark.parametrize("n", NS)
def test_pack_and_unpack_equal_the_restatement(T, n):
    torch, D, L = T
    combo = 0
    seen = np.zeros(M.RECORD, dtype=np.int64)
    for dist in DISTS:
        for cap in sorted({1, 64, 100, max(n, 1)}):
            for npayload in (0, 4):
                for axis in (M.AXIS_X, M.AXIS_Y):
                    has = ((1, 1), (1, 1), (1, 0), (0, 1))[combo % 4] if dist in ("specials", "no_free") else (1, 1)
                    c = pack_unpack_case(torch, L, dist, n, cap, npayload, axis, has, 1000 * n + combo)
                    for k in range(3):                               # sent, held, arrived of this axis
                        seen[k] += c[4 * k + 2 * axis:4 * k + 2 * axis + 2].sum()
                    seen[3] += c[M.DROPPED] - (2 if axis == M.AXIS_Y else 0)
                    combo += 1
    if n >= 255:                                                     # the cases sent, held, delivered and dropped
        assert seen[:4].min() > 0, seen[:4]


@pytest.mark.parametrize("classes", [2, 1])
def test_just_past_the_multi_block_scan(T, classes):
    """the table of the pack has two entries a block and that of the unpack one, and a scan block takes 2048 entries: the
    first n at which each needs the three-kernel scan, plus a few slots into the next tile"""
    torch, D, L = T
    n = M.first_multiblock_n(classes) + 7
    assert n > (2048 // classes - 1) * 4096 and n < (2048 // classes) * 4096 + 8
    b = [C.c_longlong(), C.c_longlong()]
    assert L.dlesm_migrate_scratch(n, C.byref(b[0])) == 0 and L.dlesm_migrate_scratch(n - 8, C.byref(b[1])) == 0
    for axis, cap in ((M.AXIS_X, 100), (M.AXIS_Y, n)):
        c = pack_unpack_case(torch, L, "specials", n, cap, 0 if cap == n else 1, axis, (1, 1), 77 + classes)
        assert c[2 * axis] > 0 and c[8 + 2 * axis] > 0


@pytest.mark.parametrize("axis", [M.AXIS_X, M.AXIS_Y])
def test_a_bad_header_count_unpacks_nothing(T, axis):
    torch, D, L = T
    n, cap = 5000, 64
    host = make_set("specials", n, axis, 2, 5)
    for which, count in ((0, -1), (1, cap + 1), (0, 2 ** 40), (1, -2 ** 63)):
        counts = [3, 3]
        counts[which] = count
        recv = make_recv(cap, 2, 9, counts=counts)
        M.field(recv[which], cap, 0)[:] = M.SENTINEL
        dev = Dev(torch, L, host, cap, recv, first_counts(axis))
        assert dev.unpack(L, axis) == 0, L.dlesm_last_error()
        want = [a.copy() for a in host[:4]] + [[a.copy() for a in host[4]]]
        c = first_counts(axis)
        M.unpack_vector(axis, BOX, *want, cap, recv, c)
        torch.cuda.synchronize()
        assert dev.equals(want, None, c) is None
        assert c[M.BAD] == 1 << (2 * axis + which) and c[8 + 2 * axis + which] == 0 and c[8 + 2 * axis + 1 - which] == 3
    recv = make_recv(cap, 2, 9, counts=[-1, cap + 1])                 # both bad: nothing is unpacked at all
    dev = Dev(torch, L, host, cap, recv, first_counts(axis))
    assert dev.unpack(L, axis) == 0
    torch.cuda.synchronize()
    got = dev.counts.cpu().numpy()
    assert got[M.BAD] == 3 << (2 * axis) and (got[8 + 2 * axis:10 + 2 * axis] == 0).all()
    assert DN.same(dev.px.cpu().numpy()[:n], host[0]) and (dev.st.cpu().numpy()[:n] == host[2]).all()


# ---------------------------------------------------------------------------------------------- the World on the device
class DeviceWorld:
    """the numpy World's ranks on the device: its slots copied up, its windows of the flow as device arrays, the real step, the
    real pack and unpack, the messages routed by torch copies"""

    def __init__(self, torch, L, w):
        self.torch, self.L, self.w = torch, L, w
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.flow = [[up(a) for a in f] for f in w.flow]
        self.sets = []
        for r in range(len(w.tiles)):
            host = (w.px[r], w.py[r], w.st[r], w.ids[r], w.payload[r])
            empty = [M.empty_message(w.cap, w.npayload) for _ in range(2)]
            self.sets.append(Dev(torch, L, host, w.cap, empty, w.counts[r]))

    def advect(self, h, nsub=1):
        for r, t in enumerate(self.w.tiles):
            tm, dx, dy, un, vn = self.flow[r]
            s = self.sets[r]
            ny, ld = t["shape"]
            rc = self.L.dlesm_drifter_step_f64(C.c_double(h), nsub, ld, ny, *t["box"], _ptr(tm), _ptr(dx), _ptr(dy), _ptr(un),
                                               _ptr(vn), s.n, _ptr(s.px), _ptr(s.py), _ptr(s.st), None)
            assert rc == 0, self.L.dlesm_last_error()

    def migrate(self):
        w = self.w
        for axis in (M.AXIS_X, M.AXIS_Y):
            for r, t in enumerate(w.tiles):
                nb, sx, sy = w.links[r]
                for m in self.sets[r].send:
                    m.fill_(int(M.SENTINEL.view(np.int64)))
                rc = self.sets[r].pack(self.L, axis, [nb[2 * axis] >= 0, nb[2 * axis + 1] >= 0], sx[2 * axis:2 * axis + 2],
                                       sy[2 * axis:2 * axis + 2], box=t["box"])
                assert rc == 0, self.L.dlesm_last_error()
            for r, t in enumerate(w.tiles):
                nb = w.links[r][0]
                for d in range(2):
                    o = nb[2 * axis + d]
                    if o >= 0:
                        self.sets[r].recv[d].copy_(self.sets[o].send[1 - d])
                    else:
                        self.sets[r].recv[d][:2] = 0
            for r, t in enumerate(w.tiles):
                assert self.sets[r].unpack(self.L, axis, box=t["box"]) == 0, self.L.dlesm_last_error()

    def differs(self):
        self.torch.cuda.synchronize()
        for r in range(len(self.w.tiles)):
            w = self.w
            bad = self.sets[r].equals((w.px[r], w.py[r], w.st[r], w.ids[r], w.payload[r]), None, w.counts[r])
            if bad:
                return "rank %d: %s" % (r, bad)
        return None


@pytest.mark.parametrize("mesh", [(2, 2), (3, 2)], ids=lambda m: "%dx%d" % m)
def test_the_world_on_the_device_equals_the_numpy_world(T, mesh):
    torch, D, L = T
    nx, ny, steps = 96, 80, 30
    flow = M.gyre(nx, ny)
    rng = np.random.default_rng(21)
    x, y = 2.0 + nx * rng.random(20000), 2.0 + ny * rng.random(20000)
    w = M.World(flow, M.make_tiles(nx, ny, *mesh), mesh, nslots=12288, cap=48, x=x, y=y, npayload=2)
    dw = DeviceWorld(torch, L, w)
    moved = 0
    for step in range(steps):
        w.advect(400.0), dw.advect(400.0)
        assert dw.differs() is None, "the step itself differs"
        w.migrate(), dw.migrate()
        bad = dw.differs()
        assert bad is None, (step, bad)
        moved += sum(int(c[0:4].sum()) for c in w.counts)
        assert all(c[M.DROPPED] == 0 and c[M.BAD] == 0 for c in w.counts)
    assert sorted(w.census()) == list(range(20000))
    assert moved > 1000 and w.held > 0


@pytest.mark.parametrize("mesh", [(2, 2), (3, 2)], ids=lambda m: "%dx%d" % m)
def test_the_lattice_flow_equals_the_undivided_step_on_the_device(T, mesh):
    torch, D, L = T
    nx, ny, steps = 48, 40, 44
    flow, isl = M.lattice(nx, ny)
    x, y = M.lattice_seeds(nx, ny, isl, steps)
    n = len(x)
    w = M.World(flow, M.make_tiles(nx, ny, *mesh), mesh, nslots=2048, cap=64, x=x, y=y)
    dw = DeviceWorld(torch, L, w)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    G = [up(a) for a in flow]
    gx, gy, gst = up(x), up(y), torch.zeros(n, dtype=torch.int32, device="cuda")
    crossed = 0
    for step in range(steps):
        assert L.dlesm_drifter_step_f64(C.c_double(250.0), 1, nx + 2, ny + 2, 2, nx + 1, 2, ny + 1, *[_ptr(a) for a in G], n,
                                        _ptr(gx), _ptr(gy), _ptr(gst), None) == 0
        dw.advect(250.0), dw.migrate()
        torch.cuda.synchronize()
        hx, hy, hst = gx.cpu().numpy(), gy.cpu().numpy(), gst.cpu().numpy()
        seen = {}
        for r, t in enumerate(w.tiles):
            s = dw.sets[r]
            px, py, st, ids = (a.cpu().numpy()[:s.n] for a in (s.px, s.py, s.st, s.ids))
            live = st != M.FREE
            for i, a, b, c in zip(ids[live], st[live], px[live] + t["off"][0], py[live] + t["off"][1]):
                assert int(i) not in seen
                seen[int(i)] = (a, b, c)
            crossed += int(s.counts[0:4].sum())
        assert sorted(seen) == list(range(n))
        assert (np.array([seen[i][0] for i in range(n)]) == hst).all(), step
        assert DN.same(np.array([seen[i][1] for i in range(n)]), hx) and DN.same(np.array([seen[i][2] for i in range(n)]), hy), step
    assert crossed > 300 and set(hst.tolist()) == {DN.ACTIVE, DN.LEFT, DN.GROUNDED}


def test_one_rank_as_its_own_neighbour_is_a_periodic_channel(T):
    """dlesm_migrate_f64 with the caller's own rank on the W and E side and shifts of a box width: a uniform eastward flow
    carries the particles round and round; against the numpy World with the same links"""
    torch, D, L = T
    nx, ny, steps, n, cap = 24, 6, 40, 512, 6
    flow, _ = M.lattice(nx, ny)
    flow = (np.ones_like(flow[0]), flow[1], flow[2], 3.0 * flow[3], 0.0 * flow[4])       # 3/4 of a cell a step, no island
    rng = np.random.default_rng(3)
    x, y = 2.0 + rng.integers(0, 8 * nx, 300) / 8.0, 2.0 + rng.integers(0, 8 * ny, 300) / 8.0
    tiles = M.make_tiles(nx, ny, 1, 1)
    w = M.World(flow, tiles, (1, 1), nslots=n, cap=cap, x=x, y=y, npayload=1)
    w.links = [([0, 0, -1, -1], [nx, -nx, 0, 0], [0, 0, 0, 0])]
    dw = DeviceWorld(torch, L, w)
    s = dw.sets[0]
    need = C.c_longlong()
    assert L.dlesm_migrate_work(n, cap, 1, C.byref(need)) == 0
    work = torch.full((need.value + GUARD,), BYTE_FILL, dtype=torch.uint8, device="cuda")
    rounds = 0
    for step in range(steps):
        w.advect(250.0), dw.advect(250.0)
        w.migrate()
        rc = L.dlesm_migrate_f64(*tiles[0]["box"], n, _ptr(s.px), _ptr(s.py), _ptr(s.st), _ptr(s.ids), _pp(s.payload), 1,
                                 _i2(w.links[0][0]), _i2(w.links[0][1]), _i2(w.links[0][2]), cap, _ptr(s.counts), _ptr(work),
                                 need.value, None)
        assert rc == 0, L.dlesm_last_error()
        bad = dw.differs()
        assert bad is None, (step, bad)
        rounds += int(w.counts[0][M.E])
        assert w.counts[0][M.E] == w.counts[0][8 + M.W] and w.counts[0][M.DROPPED] == 0
    assert bool((work[need.value:] == BYTE_FILL).all())
    assert rounds > 150 and w.held > 0 and sorted(w.census()) == list(range(300))
    assert (w.st[0] == M.ACTIVE).sum() + (w.st[0] == M.LEFT).sum() == 300


def test_captured_into_a_graph_and_on_two_streams(T):
    torch, D, L = T
    n, cap, axis = 9000, 40, M.AXIS_X
    hosts = [make_set("specials", n, axis, 2, 50 + k) for k in range(4)]
    recv = make_recv(cap, 2, 60)
    dev = Dev(torch, L, hosts[0], cap, recv, first_counts(axis))
    has, sx, sy = (1, 1), (38, -38), (0, 0)

    def want_of(host):
        want = [a.copy() for a in host[:4]] + [[a.copy() for a in host[4]]]
        send = [M.new_message(cap, 2) for _ in range(2)]
        c = first_counts(axis)
        M.pack_vector(axis, BOX, *want, has, sx, sy, cap, send, c)
        M.unpack_vector(axis, BOX, *want, cap, recv, c)
        return want, send, c

    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        assert dev.pack(L, axis, has, sx, sy, stream=side) == 0, L.dlesm_last_error()
        assert dev.unpack(L, axis, stream=side) == 0, L.dlesm_last_error()
    for host in hosts[1:]:                                           # three replays, each on other data
        for t, a in zip([dev.px, dev.py, dev.st, dev.ids] + dev.payload, list(host[:4]) + host[4]):
            t[:n].copy_(torch.from_numpy(np.array(a)))
        for m in dev.send:
            m.fill_(int(M.SENTINEL.view(np.int64)))
        dev.counts.fill_(-9)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert dev.equals(*want_of(host)) is None
    # two sets on two streams at once
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    devs = [Dev(torch, L, hosts[k], cap, recv, first_counts(axis)) for k in range(2)]
    torch.cuda.synchronize()
    for k in range(2):
        assert devs[k].pack(L, axis, has, sx, sy, stream=streams[k]) == 0
    for k in range(2):
        assert devs[k].unpack(L, axis, stream=streams[k]) == 0
    torch.cuda.synchronize()
    for k in range(2):
        assert devs[k].equals(*want_of(hosts[k])) is None


def test_the_python_wrapper_on_a_single_rank_grid(T):
    """no neighbours: nothing moves, the LEFT stay LEFT, nfree is the FREE slots; the thin wrappers equal the restatement"""
    torch, D, L = T
    g = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
    g.decompose(38, 20)
    D.grid_init(g, 1000.0, 1000.0)
    it = g.subdomain.internal
    box = (it.xstart, it.xstop, it.ystart, it.ystop)
    un = D.r2d_field(g, D.GO_U_POINTS)
    n = 3000
    host = make_set("specials", n, M.AXIS_X, 1, 8)
    up = lambda a: torch.from_numpy(np.array(a)).cuda()
    px, py, st, ids, pay = up(host[0]), up(host[1]), up(host[2]), up(host[3]), up(host[4][0])
    assert D.psy.migrate_neighbours(g) == ([-1] * 4, [0] * 4, [0] * 4)
    for target in (g, un):
        rec = D.particle_migrate(px, py, st, ids, target, payload=[pay], cap=50)
        assert isinstance(rec, D._cabi.MigrateCounts)
        assert rec.as16() == (0,) * 13 + (int((host[2] == M.FREE).sum()), 0, 0)
    assert DN.same(px.cpu().numpy(), host[0]) and (st.cpu().numpy() == host[2]).all() and (ids.cpu().numpy() == host[3]).all()
    with pytest.raises(D.DlesmError):
        D.particle_migrate(px, py, st, ids.int(), g)
    with pytest.raises(D.DlesmError):
        D.particle_migrate(px, py, st, ids, g, payload=[pay] * 5)
    # the thin wrappers: pack, a device copy as the exchange of a rank that is its own neighbour, unpack
    cap = 64
    send = [D.migrate_message(cap, 1) for _ in range(2)]
    recv = [D.migrate_message(cap, 1) for _ in range(2)]
    counts = torch.full((16,), -9, dtype=torch.int32, device="cuda")
    D.particle_pack(M.AXIS_X, px, py, st, ids, BOX, (1, 1), (38, -38), (0, 0), cap, send, counts, payload=[pay])
    D.particle_exchange([0, 0], send, recv)
    D.particle_unpack(M.AXIS_X, px, py, st, ids, BOX, cap, recv, counts, payload=[pay])
    torch.cuda.synchronize()
    want = [a.copy() for a in host[:4]] + [[host[4][0].copy()]]
    hs, c = [M.new_message(cap, 1) for _ in range(2)], np.full(M.RECORD, -9, dtype=np.int32)
    M.pack_vector(M.AXIS_X, BOX, *want, (1, 1), (38, -38), (0, 0), cap, hs, c)
    M.unpack_vector(M.AXIS_X, BOX, *want, cap, [hs[1], hs[0]], c)
    assert DN.same(px.cpu().numpy(), want[0]) and (st.cpu().numpy() == want[2]).all() and (counts.cpu().numpy() == c).all()
    assert (pay.cpu().numpy().view(np.uint64) == want[4][0].view(np.uint64)).all() and c[M.E] > 0 and c[8 + M.W] == c[M.E]
    D.particle_exchange([-1, -1], send, recv)                         # no neighbour: empty messages
    assert int(recv[0][:8].view(torch.int64)[0]) == 0 and int(recv[1][:8].view(torch.int64)[0]) == 0
