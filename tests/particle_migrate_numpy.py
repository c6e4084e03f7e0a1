"""CPU restatements of the particle migration and a World that runs R ranks in one process.

pack_scalar / unpack_scalar walk the slots one at a time through the rule as it is written; pack_vector / unpack_vector do
the same with cumsum and boolean masks and never loop over slots.  Both work in place.  A message is a uint64 array of
2 + (3 + npayload) * cap words: count, padding, x[cap] | y[cap] | id[cap] | payload_k[cap], doubles as their bits.  The record
is an int32 array of 16: sent[4] held[4] arrived[4] dropped nfree bad_message pad, directions W, E, S, N.

World: R tiles of one global flow, each with its window of the arrays in its own local frame, its slots and its messages; a
step is drifter_numpy's step per rank and then both phases with the messages routed by hand.
"""
import numpy as np

import drifter_numpy as DN

ACTIVE, LEFT, OPEN, GROUNDED, FREE = range(5)
W, E, S, N = range(4)
AXIS_X, AXIS_Y = 0, 1
MAX_PAYLOAD = 4
TILE, SCAN_TILE = 4096, 2048           # slots of a block; table entries of a scan block (the plan's constants)
RECORD = 16
DROPPED, NFREE, BAD, PAD = 12, 13, 14, 15
SENTINEL = np.uint64(0xA5A5A5A5DEADBEEF)
F = np.float64


def message_words(cap, npayload):
    return 2 + (3 + npayload) * cap


def new_message(cap, npayload, fill=SENTINEL):
    return np.full(message_words(cap, npayload), fill, dtype=np.uint64)


def empty_message(cap, npayload):
    m = new_message(cap, npayload)
    m[0] = 0
    return m


def field(msg, cap, w):
    """array w (0: x, 1: y, 2: id, 3 + k: payload k) of a message, as a uint64 view"""
    return msg[2 + w * cap:2 + (w + 1) * cap]


def first_multiblock_n(classes=2):
    """the smallest n whose table of classes x nblocks + 1 entries, padded to eight, is more than one scan block"""
    nblocks = 1
    while -(-(classes * nblocks + 1) // 8) * 8 <= SCAN_TILE:
        nblocks += 1
    return (nblocks - 1) * TILE + 1


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ---------------------------------------------------------------------------------------------- one slot at a time
def _class_scalar(axis, box, x, y, has):
    xs, xe, ys, ye = box
    if not (np.isfinite(x) and np.isfinite(y)):
        return 0
    if axis == AXIS_X:
        if x < F(xs):
            return 1 if has[0] else 0
        if x >= F(xe) + F(1.0):
            return 2 if has[1] else 0
        return 0
    if not (x >= F(xs) and x < F(xe) + F(1.0)):
        return 0
    if y < F(ys):
        return 1 if has[0] else 0
    if y >= F(ye) + F(1.0):
        return 2 if has[1] else 0
    return 0


def pack_scalar(axis, box, px, py, status, ids, payload, has, shift_x, shift_y, cap, send, counts):
    k = [0, 0]
    for p in range(len(px)):
        if status[p] != LEFT:
            continue
        c = _class_scalar(axis, box, px[p], py[p], has)
        if c == 0:
            continue
        d = c - 1
        if k[d] < cap:
            field(send[d], cap, 0)[k[d]] = _bits(np.array([px[p] + F(shift_x[d])]))[0]
            field(send[d], cap, 1)[k[d]] = _bits(np.array([py[p] + F(shift_y[d])]))[0]
            field(send[d], cap, 2)[k[d]] = _bits(ids)[p]
            for q, a in enumerate(payload):
                field(send[d], cap, 3 + q)[k[d]] = _bits(a)[p]
            status[p] = FREE
        k[d] += 1
    for d in range(2):
        send[d][0] = min(k[d], cap)
        counts[2 * axis + d] = min(k[d], cap)
        counts[4 + 2 * axis + d] = k[d] - min(k[d], cap)


def _header(msg, cap, axis, d):
    c = int(msg[:1].view(np.int64)[0])
    if c < 0 or c > cap:
        return 0, 1 << (2 * axis + d)
    return c, 0


def unpack_scalar(axis, box, px, py, status, ids, payload, cap, recv, counts):
    c0, b0 = _header(recv[0], cap, axis, 0)
    c1, b1 = _header(recv[1], cap, axis, 1)
    j = 0
    arrived = [0, 0]
    for p in range(len(px)):
        if j >= c0 + c1:
            break
        if status[p] != FREE:
            continue
        d, k = (0, j) if j < c0 else (1, j - c0)
        x = field(recv[d], cap, 0)[k:k + 1].view(np.float64)[0]
        y = field(recv[d], cap, 1)[k:k + 1].view(np.float64)[0]
        px[p], py[p] = x, y
        _bits(ids)[p] = field(recv[d], cap, 2)[k]
        for q, a in enumerate(payload):
            _bits(a)[p] = field(recv[d], cap, 3 + q)[k]
        status[p] = ACTIVE if DN.inbox(box, x, y) else LEFT
        arrived[d] += 1
        j += 1
    dropped = c0 + c1 - j
    counts[8 + 2 * axis], counts[8 + 2 * axis + 1] = arrived
    if axis == AXIS_X:
        counts[DROPPED], counts[BAD], counts[PAD] = dropped, b0 | b1, 0
    else:
        counts[DROPPED] += dropped
        counts[BAD] |= b0 | b1
    counts[NFREE] = int(np.count_nonzero(status == FREE))


# ---------------------------------------------------------------------------------------------- all slots at once
def pack_vector(axis, box, px, py, status, ids, payload, has, shift_x, shift_y, cap, send, counts):
    xs, xe, ys, ye = box
    with np.errstate(invalid="ignore"):
        cand = (status == LEFT) & np.isfinite(px) & np.isfinite(py)
        if axis == AXIS_X:
            lo, hi = cand & (px < xs), cand & (px >= xe + 1.0)
        else:
            inx = (px >= xs) & (px < xe + 1.0)
            lo, hi = cand & inx & (py < ys), cand & inx & (py >= ye + 1.0)
    for d, m in enumerate((lo, hi)):
        m = m & bool(has[d])
        rank = np.cumsum(m) - 1
        go = m & (rank < cap)
        k = rank[go]
        field(send[d], cap, 0)[k] = _bits(px[go] + float(shift_x[d]))
        field(send[d], cap, 1)[k] = _bits(py[go] + float(shift_y[d]))
        field(send[d], cap, 2)[k] = _bits(ids)[go]
        for q, a in enumerate(payload):
            field(send[d], cap, 3 + q)[k] = _bits(a)[go]
        status[go] = FREE
        total = int(np.count_nonzero(m))
        send[d][0] = min(total, cap)
        counts[2 * axis + d] = min(total, cap)
        counts[4 + 2 * axis + d] = total - min(total, cap)


def unpack_vector(axis, box, px, py, status, ids, payload, cap, recv, counts):
    c0, b0 = _header(recv[0], cap, axis, 0)
    c1, b1 = _header(recv[1], cap, axis, 1)
    slots = np.flatnonzero(status == FREE)
    take = slots[:c0 + c1]
    a0 = min(c0, len(take))
    a1 = len(take) - a0
    x = np.concatenate([field(recv[0], cap, 0)[:a0], field(recv[1], cap, 0)[:a1]]).view(np.float64)
    y = np.concatenate([field(recv[0], cap, 1)[:a0], field(recv[1], cap, 1)[:a1]]).view(np.float64)
    px[take], py[take] = x, y
    _bits(ids)[take] = np.concatenate([field(recv[0], cap, 2)[:a0], field(recv[1], cap, 2)[:a1]])
    for q, a in enumerate(payload):
        _bits(a)[take] = np.concatenate([field(recv[0], cap, 3 + q)[:a0], field(recv[1], cap, 3 + q)[:a1]])
    status[take] = np.where(DN._inbox_v(box, x, y), ACTIVE, LEFT)
    counts[8 + 2 * axis], counts[8 + 2 * axis + 1] = a0, a1
    dropped = c0 + c1 - len(take)
    if axis == AXIS_X:
        counts[DROPPED], counts[BAD], counts[PAD] = dropped, b0 | b1, 0
    else:
        counts[DROPPED] += dropped
        counts[BAD] |= b0 | b1
    counts[NFREE] = len(slots) - len(take)


# ---------------------------------------------------------------------------------------------- flows
def gyre(nx, ny, island=True, seed=621):
    """(tm, dx_t, dy_t, un, vn) of (ny + 2) x (nx + 2): a closed basin (land ring) with one anticlockwise gyre, a little noise,
    and an island across the middle, where tiles of 2 x 2 and 3 x 2 meshes meet"""
    rng = np.random.default_rng(seed)
    gny, gld = ny + 2, nx + 2
    tm = np.ones((gny, gld), dtype=np.int32)
    tm[0, :] = tm[-1, :] = 0
    tm[:, 0] = tm[:, -1] = 0
    if island:
        tm[gny // 2 - 4:gny // 2 + 3, gld // 2 - 5:gld // 2 + 4] = 0
    jj, ii = np.mgrid[1:gny + 1, 1:gld + 1]
    xc, yc = (ii - 0.5 * gld) / (0.5 * nx), (jj - 0.5 * gny) / (0.5 * ny)
    un = -1.4 * yc * (1.0 - xc * xc) + 0.3 * (rng.random((gny, gld)) - 0.5)
    vn = 1.4 * xc * (1.0 - yc * yc) + 0.3 * (rng.random((gny, gld)) - 0.5)
    dx_t = 900.0 + 200.0 * rng.random((gny, gld))
    dy_t = 900.0 + 200.0 * rng.random((gny, gld))
    return tm, dx_t, dy_t, un, vn


def lattice(nx, ny):
    """the lattice flow: no land but one island, un = 1, vn = 0.5, dx = dy = 1000 (with h = 250 a step moves (1/4, 1/8))"""
    gny, gld = ny + 2, nx + 2
    tm = np.ones((gny, gld), dtype=np.int32)
    isl = (slice(gny // 2 - 3, gny // 2 + 2), slice(gld // 2 - 3, gld // 2 + 3))
    tm[isl] = 0
    one = np.ones((gny, gld))
    return (tm, 1000.0 * one, 1000.0 * one, 1.0 * one, 0.5 * one), isl


def lattice_seeds(nx, ny, isl, steps, h=250.0):
    """start positions on multiples of 1/8 whose whole path lies in uniform flow, plus some on the island.  Next to the island
    a face is switched off and a cell's velocity is linear in the position: each step there adds five significant bits, after
    nine the sums round, and they round differently in a tile's frame and in the global one.  So a seed is kept when no
    position of its undisturbed path -- a straight line, (1/4, 1/8) a step -- comes within one and a half cells of the
    island; the seeds on the island are GROUNDED by the entry test and never move."""
    rng = np.random.default_rng(6211)
    x = 2.0 + rng.integers(0, 8 * nx, 4000) / 8.0
    y = 2.0 + rng.integers(0, 8 * ny, 4000) / 8.0
    y0, y1, x0, x1 = isl[0].start + 1, isl[0].stop + 1, isl[1].start + 1, isl[1].stop + 1      # the island: [x0, x1) x [y0, y1)
    on = (x >= x0) & (x < x1) & (y >= y0) & (y < y1)
    t = np.arange(steps + 1)[:, None]
    xt, yt = x[None, :] + 0.25 * t, y[None, :] + 0.125 * t
    near = ((xt >= x0 - 1.5) & (xt < x1 + 1.5) & (yt >= y0 - 1.5) & (yt < y1 + 1.5)).any(axis=0)
    keep = on | ~near
    return x[keep], y[keep]


# ---------------------------------------------------------------------------------------------- the World
def split(n, parts):
    """the first and last index, 0-based, of `parts` near-equal runs of 0..n-1"""
    edges = [(n * k) // parts for k in range(parts + 1)]
    return [(edges[k], edges[k + 1] - 1) for k in range(parts)]


def make_tiles(nx, ny, mx, my):
    """tiles of the nx x ny internal region of the (ny + 2) x (nx + 2) global array, rank = iy * mx + ix; each has its box in
    a frame of its own that starts at local cell 2, off = (ox, oy) with x_global = x_local + ox (global: 1-based, ring
    included), and the shape of its window"""
    tiles = []
    for (j0, j1) in split(ny, my):
        for (i0, i1) in split(nx, mx):
            w, h = i1 - i0 + 1, j1 - j0 + 1
            tiles.append(dict(box=(2, w + 1, 2, h + 1), off=(i0, j0), shape=(h + 2, w + 2)))
    return tiles


def window(glob, tile, fill=0):
    """the tile's window of a global array (cells beyond it: fill)"""
    ny, nx = tile["shape"]
    ox, oy = tile["off"]
    out = np.full((ny, nx), fill, dtype=glob.dtype)
    y0, x0 = max(0, -oy), max(0, -ox)
    y1, x1 = min(ny, glob.shape[0] - oy), min(nx, glob.shape[1] - ox)
    out[y0:y1, x0:x1] = glob[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


def neighbours(tiles, mx, my):
    """per rank: (neighbour[4], shift_x[4], shift_y[4]) in the order W, E, S, N; -1: the edge of the global domain"""
    out = []
    for r, t in enumerate(tiles):
        ix, iy = r % mx, r // mx
        nb = [r - 1 if ix > 0 else -1, r + 1 if ix < mx - 1 else -1, r - mx if iy > 0 else -1, r + mx if iy < my - 1 else -1]
        sx = [t["off"][0] - tiles[o]["off"][0] if o >= 0 else 0 for o in nb]
        sy = [t["off"][1] - tiles[o]["off"][1] if o >= 0 else 0 for o in nb]
        out.append((nb, sx, sy))
    return out


class World:
    def __init__(self, flow, tiles, mesh, nslots, cap, x, y, ids=None, npayload=0, pack=pack_vector, unpack=unpack_vector):
        self.tiles, self.mesh, self.cap, self.npayload = tiles, mesh, cap, npayload
        self.pack, self.unpack = pack, unpack
        self.links = neighbours(tiles, *mesh)
        self.flow = [tuple(window(a, t) for a in flow) for t in tiles]
        ids = np.arange(len(x), dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
        self.px, self.py, self.st, self.ids, self.payload, self.counts = [], [], [], [], [], []
        placed = np.zeros(len(x), dtype=bool)
        for t in tiles:
            ox, oy = t["off"]
            mine = DN._inbox_v(t["box"], x - ox, y - oy) & ~placed
            placed |= mine
            k = int(np.count_nonzero(mine))
            assert k <= nslots, "a tile holds more seeds than slots"
            px, py = np.full(nslots, -777.25), np.full(nslots, -777.25)
            st, idr = np.full(nslots, FREE, dtype=np.int32), np.full(nslots, -1, dtype=np.int64)
            # the seeds take every other slot from the front, then the rest in order: FREE slots lie between particles
            slots = np.concatenate([np.arange(0, nslots, 2), np.arange(1, nslots, 2)])[:k]
            slots.sort()
            px[slots], py[slots], st[slots], idr[slots] = x[mine] - ox, y[mine] - oy, ACTIVE, ids[mine]
            self.px.append(px), self.py.append(py), self.st.append(st), self.ids.append(idr)
            # payloads that can be checked: the id's bits turned round, and the start position's x
            pay = [(idr * (q + 3)).astype(np.int64) if q % 2 == 0 else np.where(idr >= 0, idr * 0.5 + q, -1.0)
                   for q in range(npayload)]
            self.payload.append(pay)
            self.counts.append(np.full(RECORD, -9, dtype=np.int32))
        assert placed.all(), "a seed lies in no tile"
        self.held = 0

    def advect(self, h, nsub=1):
        for r, t in enumerate(self.tiles):
            DN.drifter_step(h, nsub, t["box"], *self.flow[r], self.px[r], self.py[r], self.st[r])

    def migrate(self):
        R = len(self.tiles)
        for axis in (AXIS_X, AXIS_Y):
            send = [[new_message(self.cap, self.npayload) for _ in range(2)] for _ in range(R)]
            for r, t in enumerate(self.tiles):
                nb, sx, sy = self.links[r]
                self.pack(axis, t["box"], self.px[r], self.py[r], self.st[r], self.ids[r], self.payload[r],
                          [nb[2 * axis] >= 0, nb[2 * axis + 1] >= 0], sx[2 * axis:2 * axis + 2], sy[2 * axis:2 * axis + 2],
                          self.cap, send[r], self.counts[r])
            for r, t in enumerate(self.tiles):
                nb = self.links[r][0]
                recv = [send[nb[2 * axis + d]][1 - d] if nb[2 * axis + d] >= 0 else empty_message(self.cap, self.npayload)
                        for d in range(2)]
                self.unpack(axis, t["box"], self.px[r], self.py[r], self.st[r], self.ids[r], self.payload[r], self.cap, recv,
                            self.counts[r])
        self.held += sum(int(c[4:8].sum()) for c in self.counts)

    def step(self, h, nsub=1):
        self.advect(h, nsub)
        self.migrate()

    def census(self):
        """id -> (status, x_global, y_global), asserting that no id sits in two slots"""
        seen = {}
        for r, t in enumerate(self.tiles):
            ox, oy = t["off"]
            for p in np.flatnonzero(self.st[r] != FREE):
                i = int(self.ids[r][p])
                assert i not in seen, "id %d is in two slots" % i
                seen[i] = (int(self.st[r][p]), self.px[r][p] + ox, self.py[r][p] + oy)
        return seen
