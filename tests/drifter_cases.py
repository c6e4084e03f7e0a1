"""Inputs the CPU and GPU tests of the drifters share, made once and never modified.  Nothing here
needs a GPU.

The grid is ld x ny = 26 x 22 (1-based cells below): land on the west, south and north rings, two open columns in the east
(25 and 26), a 4 x 4 island (columns 10..13, rows 8..11) and a one-cell rock at (17, 15).  un and vn are random and sheared,
the metrics random in 900..1100, h = 400 s: a substep moves a particle about half a cell.  A few cells carry hand-set values
for the hand-placed particles of PLACED, one per rule; 1000 random seeds over the whole array (and beyond it) follow them, and
POOL particles in all for the tests that need many: particles are independent, so the first n of the pool after a call are
the first n of the pool's reference.
"""
import numpy as np

import drifter_numpy as DN

LD, NY = 26, 22
H = 400.0
BOXES = [(2, 25, 2, 21), (4, 20, 3, 18)]
ISLAND = (slice(7, 11), slice(9, 13))          # rows 8..11, columns 10..13
ROCK = (14, 16)                                # (17, 15)
SENTINEL = -777.25
POOL = 70001
_MADE = {}


def mask():
    tm = np.ones((NY, LD), dtype=np.int32)
    tm[:, 24:] = -1
    tm[:, 0] = 0
    tm[0, :] = 0
    tm[-1, :] = 0
    tm[ISLAND] = 0
    tm[ROCK] = 0
    return tm


def _set(a, i, j, v):
    a[j - 1, i - 1] = v


def flow():
    """(tm, dx_t, dy_t, un, vn)"""
    if "flow" in _MADE:
        return _MADE["flow"]
    rng = np.random.default_rng(617)
    tm = mask()
    jj, ii = np.mgrid[1:NY + 1, 1:LD + 1]
    un = 1.6 * (rng.random((NY, LD)) - 0.5) + 0.04 * (jj - 11.0)
    vn = 1.6 * (rng.random((NY, LD)) - 0.5) - 0.04 * (ii - 13.0)
    dx_t = 900.0 + 200.0 * rng.random((NY, LD))
    dy_t = 900.0 + 200.0 * rng.random((NY, LD))
    # (6, 15): every face -0.0 -- the particle stays, bit for bit
    for a, i, j in ((un, 5, 15), (un, 6, 15), (vn, 6, 14), (vn, 6, 15)):
        _set(a, i, j, -0.0)
    # (9, 9), west of the island: a west face fast enough to put the midpoint ON the island
    _set(un, 8, 9, 8.0)
    _set(vn, 9, 8, 0.0), _set(vn, 9, 9, 0.0)
    # (16, 14), south-west of the rock, whose neighbours (17, 14) and (16, 15) are wet: a diagonal move into the rock
    for a, i, j in ((un, 15, 14), (un, 16, 14), (vn, 16, 13), (vn, 16, 14)):
        _set(a, i, j, 1.5)
    _set(dx_t, 16, 14, 1000.0), _set(dy_t, 16, 14, 1000.0)
    # (24, 6): fast enough to put the midpoint east of the array
    _set(un, 23, 6, 10.0), _set(un, 24, 6, 10.0), _set(dx_t, 24, 6, 1000.0)
    # (20, 10): the midpoint and the move leave the sub-box
    _set(un, 19, 10, 3.0), _set(un, 20, 10, 3.0)
    # (24, 12): the midpoint on the open column, the move into it
    _set(un, 23, 12, 1.0), _set(un, 24, 12, 1.0), _set(vn, 24, 11, 0.0), _set(vn, 24, 12, 0.0)
    _set(dx_t, 24, 12, 1000.0)
    # (6, 18): a NaN on a wet face
    _set(un, 6, 18, np.nan)
    _MADE["flow"] = (tm, dx_t, dy_t, un, vn)
    return _MADE["flow"]


def embed(a, ld, fill):
    """the 26-column array in one of leading dimension ld >= 26 (the columns added lie beyond the ring: never read)"""
    out = np.full((a.shape[0], ld), fill, dtype=a.dtype)
    out[:, :a.shape[1]] = a
    return out


# (x, y, status): one particle per rule
PLACED = [
    (6.0, 5.5, DN.ACTIVE),                                   # exactly on a face, a == 0
    (7.25, 6.0, DN.ACTIVE),                                  # b == 0
    (2.0, 2.0, DN.ACTIVE), (4.0, 3.0, DN.ACTIVE),            # the boxes' first admissible coordinates
    (float(np.nextafter(26.0, 0.0)), float(np.nextafter(22.0, 0.0)), DN.ACTIVE),    # ... and their last
    (float(np.nextafter(21.0, 0.0)), float(np.nextafter(19.0, 0.0)), DN.ACTIVE),
    (float(np.nextafter(2.0, 0.0)), 5.5, DN.ACTIVE), (26.0, 5.5, DN.ACTIVE),        # one ulp outside, and on the far edge
    (6.3, 15.6, DN.ACTIVE),                                  # -0.0 velocities
    (9.5, 9.5, DN.ACTIVE),                                   # midpoint on land, the Euler move too: GROUNDED
    (16.8, 14.8, DN.ACTIVE),                                 # the diagonal move into the rock: GROUNDED
    (24.5, 6.5, DN.ACTIVE),                                  # midpoint outside the array: LEFT
    (20.5, 10.5, DN.ACTIVE),                                 # midpoint and move outside the sub-box
    (24.9, 12.5, DN.ACTIVE),                                 # midpoint on an open cell, the move into it: OPEN
    (float("nan"), 5.5, DN.ACTIVE), (5.5, float("inf"), DN.ACTIVE), (float("-inf"), 5.5, DN.ACTIVE),
    (6.5, 18.5, DN.ACTIVE),                                  # a NaN velocity on a wet face: LEFT at a NaN
    (11.5, 9.5, DN.ACTIVE), (17.5, 15.5, DN.ACTIVE),         # seeded on the island and on the rock
    (25.5, 9.5, DN.ACTIVE),                                  # seeded on an open cell
    (SENTINEL, SENTINEL, DN.LEFT), (SENTINEL, 5.5, DN.OPEN), (5.5, SENTINEL, DN.GROUNDED),   # not ACTIVE: untouched
    (5.5, 5.5, 7),                                           # (no status of the rule: untouched as well)
]
NSEEDS = 1000
NSCALAR = len(PLACED) + NSEEDS


def particles():
    """(px, py, status) of the pool: PLACED, the 1000 seeds over the array and half a cell beyond it, then seeds over the
    interior -- one in sixteen of those not ACTIVE"""
    if "pool" not in _MADE:
        rng = np.random.default_rng(6170)
        n = POOL - len(PLACED)
        x = np.where(np.arange(n) < NSEEDS, 0.5 + 27.0 * rng.random(n), 2.0 + 23.0 * rng.random(n))
        y = np.where(np.arange(n) < NSEEDS, 0.5 + 23.0 * rng.random(n), 2.0 + 19.0 * rng.random(n))
        st = np.where((np.arange(n) >= NSEEDS) & (rng.random(n) < 1 / 16), rng.integers(1, 4, n), 0)
        px = np.concatenate([[p[0] for p in PLACED], x])
        py = np.concatenate([[p[1] for p in PLACED], y])
        status = np.concatenate([[p[2] for p in PLACED], st]).astype(np.int32)
        _MADE["pool"] = (px, py, status)
    return _MADE["pool"]


def reference(box, nsub, calls=1):
    """the pool after `calls` calls with nsub substeps by the array restatement; made once"""
    key = ("ref", tuple(box), nsub, calls)
    if key not in _MADE:
        px, py, st = (a.copy() for a in particles())
        for _ in range(calls):
            DN.drifter_step(H, nsub, box, *flow(), px, py, st)
        _MADE[key] = (px, py, st)
    return _MADE[key]


def scalar_reference(box, nsub):
    """the first NSCALAR particles after one call by the scalar restatement; made once (the census with it)"""
    key = ("scalar", tuple(box), nsub)
    if key not in _MADE:
        px, py, st = (a[:NSCALAR].copy() for a in particles())
        seen = {}
        DN.drifter_step_scalar(H, nsub, box, *flow(), px, py, st, seen)
        _MADE[key] = (px, py, st, seen)
    return _MADE[key]


def sample_fields(nfields):
    rng = np.random.default_rng(61700)
    return [rng.random((NY, LD)) for _ in range(nfields)]
