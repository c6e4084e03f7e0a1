"""The cases of the particle release that the CPU and the GPU tests share: a 13 x 11 box inside a
24 x 19 array with an island, a coast and a row of open cells; source tables with every kind of source; the FREE patterns;
the rounding edge; the tables that make the scan take its three-kernel path; the tilings of the 26 x 22 basin.  A plain
module; nothing runs on import, references are computed once and kept."""
import numpy as np

import particle_migrate_numpy as M
import release_numpy as R

LD, NY = 24, 19
BOX = (5, 17, 4, 14)                       # 13 x 11
OFFSETS = [(0, 0), (100, -3), (-3, 7)]
NS = [0, 1, 64, 4095, 4096, 4097, 12289]
PATTERNS = ["none", "all", "third", "last", "wave"]
COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1000]
SEED = 0x9E3779B97F4A7C15                  # its high word is not zero
TICK, TICK_DEV = 5, 2 ** 32 + 9
SENT_F, SENT_I, SENT_ST = -777.25, -0x5A5A5A5A5A5A5A5B, 3      # a slot that is not FREE is GROUNDED: no entry moves it
_KEPT = {}


def mask():
    """tm of NY x LD: water, with land outside the box's ring, a coast in the box's north-west, an island and open cells along
    the box's northern row"""
    tm = np.ones((NY, LD), dtype=np.int32)
    tm[:2, :] = tm[-3:, :] = 0
    tm[:, :3] = tm[:, -5:] = 0
    tm[10:14, 4:7] = 0                     # cells (5..7, 11..14): the coast
    tm[6:9, 9:12] = 0                      # cells (10..12, 7..9): the island
    tm[13, 8:15] = -1                      # cells (9..15, 14): open
    return tm


def free_pattern(n, pattern):
    st = np.full(n, SENT_ST, dtype=np.int32)
    k = np.arange(n)
    if pattern == "all":
        st[:] = R.FREE
    elif pattern == "third":
        st[k % 3 == 1] = R.FREE
    elif pattern == "last":
        st[n - 1:] = R.FREE
    elif pattern == "wave":                # one wave of the second tile only
        st[(k >= R.TILE + 1024) & (k < R.TILE + 1088)] = R.FREE
    return st


def sources(off, counts=None, shift=0):
    """one source of every kind, in global coordinates for the tile at `off`; counts cycle through COUNTS from `shift`"""
    ox, oy = off
    inf, nan = np.inf, np.nan
    rows = [  # x, y (local), rx, ry, next_id
        (8.5, 5.5, 0.0, 0.0, 0),                             # a point on water
        (11.5, 8.5, 0.0, 0.0, 5000),                         # a point on the island
        (2.5, 5.5, 0.0, 0.0, 10000),                         # a point outside the box
        (17.5, 6.0, 2.0, 1.0, 2 ** 32 - 30),                 # a patch across the eastern edge; ids carry into the high word
        (7.0, 12.0, 2.5, 1.5, 2 ** 63 - 20),                 # a patch across the coast; ids wrap
        (11.0, 14.0, 3.0, 0.9, 3 * 2 ** 32 + 17),            # a patch across the open cells and the northern edge
        (nan, 5.5, 1.0, 1.0, 20000),                         # bad: x
        (8.5, 5.5, -1.0, 1.0, 30000),                        # bad: rx
        (8.5, 5.5, 1.0, 1.0, 40000),                         # bad: count (set below)
        (8.5, inf, 1.0, 1.0, 50000),                         # bad: y
        (8.5, 5.5, 1.0, inf, 60000),                         # bad: ry
        (1e308, 5.5, 1e308, 0.0, 70000),                     # valid; gx may be infinite: nobody's
        (11.0, 9.0, 6.5, 5.5, -2 ** 40),                     # a patch over the whole box, negative ids
        (5.0, 4.0, 0.0, 0.0, 80000),                         # a point on the box's first corner
        (12.25, 4.75, 4.0, 0.25, 90000),                     # a thin patch along the southern row
    ]
    cyc = COUNTS if counts is None else counts
    count = [cyc[(k + shift) % len(cyc)] for k in range(len(rows))]
    count[8] = -1
    return R.table([r[0] + ox for r in rows], [r[1] + oy for r in rows], [r[2] for r in rows], [r[3] for r in rows],
                   [r[4] for r in rows], count)


def edge_sources():
    """offx = -3: a point source one ulp below the tile's global upper edge 15; 15 - 2^-49 + 3 is a tie that rounds to the
    even 18 = xstop + 1, the box's upper edge"""
    gx = np.nextafter(15.0, -np.inf)
    assert gx + 3.0 == 18.0 and gx < 15.0
    return R.table([gx, gx], [12.5, 12.5], [0.0, 0.0], [0.0, 0.0], [7, 1000], [1, 0])


def deep_sources(off):
    """2100 sources of one particle each: a table of more than SCAN_TILE entries"""
    rng = np.random.default_rng(623)
    ns = 2100
    x = off[0] + 3.0 + 17.0 * rng.random(ns)
    y = off[1] + 2.0 + 15.0 * rng.random(ns)
    return R.table(x, y, 0.5 * rng.random(ns), 0.5 * rng.random(ns), np.arange(ns) * 10, [1] * ns)


def case(name, off=(0, 0), n=4097, pattern="third", max_count=256, src=None, optional=True, box=BOX):
    return dict(name=name, box=box, off=off, n=n, pattern=pattern, max_count=max_count,
                sources=sources(off) if src is None else src, optional=optional, seed=SEED)


def cases():
    out = []
    for off in OFFSETS:
        for mc in (256, 1000):
            out.append(case("kinds off=%s max_count=%d" % (off, mc), off=off, n=12289, pattern="all", max_count=mc,
                            src=sources(off, shift=3)))
    k = 0
    for n in NS:
        for pattern in PATTERNS:
            out.append(case("n=%d %s" % (n, pattern), off=OFFSETS[1], n=n, pattern=pattern, max_count=(256, 1000)[k % 2],
                            src=sources(OFFSETS[1], shift=k), optional=k % 3 != 0))
            k += 1
    out.append(case("overflow", off=OFFSETS[2], n=4097, pattern="third", max_count=1000, src=sources(OFFSETS[2], counts=[1000])))
    out.append(case("edge", off=OFFSETS[2], n=64, pattern="all", max_count=1, src=edge_sources()))
    out.append(case("deep table", off=OFFSETS[1], n=4097, pattern="third", max_count=1, src=deep_sources(OFFSETS[1])))
    out.append(case("no sources", n=65, pattern="all", src=sources((0, 0))[:0]))
    out.append(case("empty box", n=65, pattern="all", box=(5, 4, 4, 14)))
    return out


def deep_slots_case():
    """the slot table alone above one scan block, few FREE slots: the first, a wave in the middle, the last"""
    n = M.first_multiblock_n(1)
    c = case("deep slots", off=OFFSETS[1], n=n, pattern=None, max_count=256)
    st = np.full(n, SENT_ST, dtype=np.int32)
    st[0] = st[n - 1] = R.FREE
    st[n // 2:n // 2 + 64] = R.FREE
    c["status"] = st
    return c


def arrays(c):
    """(px, py, status, ids, tag, born) of a case before the call, sentinels in every word"""
    n = c["n"]
    st = c["status"].copy() if "status" in c else free_pattern(n, c["pattern"])
    opt = [np.full(n, SENT_I, dtype=np.int64) if c["optional"] else None for _ in range(2)]
    return [np.full(n, SENT_F), np.full(n, SENT_F), st, np.full(n, SENT_I, dtype=np.int64)] + opt


def run(c, how=R.release_vector, arr=None, src=None, tm=None):
    """the case through a restatement: (arrays, table, record) afterwards"""
    arr = arrays(c) if arr is None else arr
    src = c["sources"].copy() if src is None else src
    rec = how(c["box"], c["off"], mask() if tm is None else tm, src, c["max_count"], c["seed"], TICK + TICK_DEV, *arr)
    return arr, src, rec


def reference(c):
    """run(c) by release_vector, computed once and never changed"""
    if c["name"] not in _KEPT:
        _KEPT[c["name"]] = run(c)
    return _KEPT[c["name"]]


# ---------------------------------------------------------------------------------------------- the tilings
BASIN = (26, 22)


def basin_mask():
    return M.gyre(*BASIN)[0]


def basin_sources(count=300):
    """sources over the 26 x 22 basin (global cells 2..27 x 2..23): patches across tile seams, the island, the basin's rim"""
    rows = [(15.0, 13.0, 12.0, 10.0, 0), (14.5, 12.5, 3.0, 3.0, 10 ** 6), (9.0 + 2.0 / 3.0, 6.0, 1.5, 4.0, 2 ** 32 - 100),
            (27.5, 23.5, 1.0, 1.0, 2 ** 33), (10.0, 13.0, 0.0, 0.0, 2 ** 34), (2.0, 2.0, 0.75, 0.75, 2 ** 35),
            (19.0 + 1.0 / 3.0, 13.0, 0.0, 5.0, 2 ** 36), (15.0, 9.0 + 1.0 / 3.0, 11.0, 0.0, 2 ** 37)]
    return R.table(*[[r[k] for r in rows] for k in range(5)], [count] * len(rows))


def tile_case(tile, src, count):
    ny, nx = tile["shape"]
    return dict(name="tile", box=tile["box"], off=tile["off"], n=len(src) * count, pattern="all", max_count=count,
                sources=src.copy(), optional=True, seed=SEED)


def census(arr, off):
    """{id: (x_global, y_global, status)} of the slots that are not FREE"""
    px, py, st, ids = arr[:4]
    live = np.flatnonzero(st != R.FREE)
    out = {int(ids[p]): (px[p] + off[0], py[p] + off[1], int(st[p])) for p in live}
    assert len(out) == len(live), "an id sits in two slots"
    return out
