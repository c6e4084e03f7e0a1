"""Inputs the CPU and GPU tests of the random walk in a varying diffusivity share, made once and never
modified: the grid, the flow, the boxes and the particle pool are those of tests/drifter_cases.py (H = 400 s), the seed, the
tick and the identities those of tests/dispersal_cases.py; here are the field kh_t, the references by the restatements of
tests/random_walk_numpy.py and the closed basin of the well-mixed test.  Nothing here needs a GPU.

kh_t on the 26 x 22 grid (1-based cells): a smooth part 40 (1 + 0.8 sin(2 pi i / 9) cos(2 pi j / 7)) m2/s, 8 to 72; a steep part,
columns 18 to 21, 2 or 150 m2/s in blocks of 2 x 2 cells laid out like a chessboard, so that a face carries 2, 76 or 150 and
the difference across a cell is up to 74 (the largest kick, sqrt(6 150 400) = 600 m, and the largest drift, 400 x 74 / 900^2 =
0.04 cells, stay within a cell); exactly 0 on the 3 x 3 wet block of columns 5 to 7, rows 4 to 6 -- in its centre both axes
have K = 0 on both faces -- and on the wet cells (14, 9) and (14, 10) east of the island; NaN on every land cell; SENTINEL in
the columns that embed() adds.  The open columns keep the smooth part: column 24 reads them.

On "the extrapolation goes negative": with values >= 0 it cannot.  kx = kw + dkx (a + cx / 2) = (kw + dkx a) + |h| dkx^2 / (2 dx^2):
the first term lies between the two face values because 0 <= a < 1, the second is >= 0 -- the drift points up the gradient, so
half a drift ahead K is larger, not smaller.  The clamp is reached with K = 0 on both faces (the census counts it) and by a
field that breaks the contract, which BAD below does on purpose: negative, infinite and NaN values on wet cells.
"""
import numpy as np

import dispersal_cases as PC
import drifter_cases as DC
import random_walk_numpy as RN

SEED, TICK, ids, signed = PC.SEED, PC.TICK, PC.ids, PC.signed
_MADE = {}


def kh_field():
    if "kh" not in _MADE:
        tm = DC.mask()
        jj, ii = np.mgrid[1:DC.NY + 1, 1:DC.LD + 1]
        kh = 40.0 * (1.0 + 0.8 * np.sin(2.0 * np.pi * ii / 9.0) * np.cos(2.0 * np.pi * jj / 7.0))
        steep = (ii >= 18) & (ii <= 21)
        kh[steep] = np.where(((ii - 18) // 2 + jj // 2) % 2 == 0, 2.0, 150.0)[steep]
        kh[3:6, 4:7] = 0.0
        kh[8:10, 13] = 0.0
        kh[tm == 0] = np.nan
        _MADE["kh"] = kh
    return _MADE["kh"]


def constant_field(kh):
    """kh on every cell that is not land, NaN on land"""
    return np.where(DC.mask() != 0, float(kh), np.nan)


def bad_field():
    """kh_field() with values the contract excludes on wet cells: negative ones, an infinity, a NaN"""
    if "bad" not in _MADE:
        kh = kh_field().copy()
        kh[11:14, 4:9] = -30.0
        kh[16, 6:9] = -1e-300
        kh[17, 14], kh[18, 14], kh[5, 15] = np.inf, np.nan, -np.inf
        _MADE["bad"] = kh
    return _MADE["bad"]


def reference(box, nsub, with_ids, field="kh", seed=SEED, tick=TICK, calls=1):
    """the pool after `calls` calls (the tick advanced by nsub between them) by the array restatement; made once.  field: "kh",
    "bad" or a number (the constant field).  Returns (px, py, status, census)"""
    key = ("ref", tuple(box), nsub, with_ids, field, seed, tick, calls)
    if key not in _MADE:
        kh = kh_field() if field == "kh" else bad_field() if field == "bad" else constant_field(field)
        px, py, st = (a.copy() for a in DC.particles())
        seen = {}
        for c in range(calls):
            RN.random_walk(DC.H, nsub, kh, seed, tick + c * nsub, box, *DC.flow(), px, py, st, ids() if with_ids else None, seen)
        _MADE[key] = (px, py, st, seen)
    return _MADE[key]


def scalar_reference(box, nsub, with_ids, field="kh"):
    """the first NSCALAR particles after one call by the scalar restatement; made once"""
    key = ("scalar", tuple(box), nsub, with_ids, field)
    if key not in _MADE:
        kh = kh_field() if field == "kh" else bad_field() if field == "bad" else constant_field(field)
        px, py, st = (a[:DC.NSCALAR].copy() for a in DC.particles())
        seen = {}
        RN.random_walk_scalar(DC.H, nsub, kh, SEED, TICK, box, *DC.flow(), px, py, st, ids()[:DC.NSCALAR] if with_ids else None,
                              seen)
        _MADE[key] = (px, py, st, seen)
    return _MADE[key]


# ---------------------------------------------------------------------------------------------- the well-mixed basin
BASIN, MESH, WM_H, WM_N, WM_STEPS, WM_SUB = 16, 1000.0, 400.0, 2 ** 14, 800, 100


def basin():
    """a closed basin of 16 x 16 wet cells of 1000 m inside a ring of land that lies in the box (a kick onto it is rejected; beyond the
    box a particle would be LEFT), still water:
    (box, tm, dx_t, dy_t, un, vn, kh_t) with K = 50 (1 + 0.9 sin(2 pi (i - 1/2) / 16)) (1 + 0.9 sin(2 pi (j - 1/2) / 16)) m2/s
    over the wet cells i, j = 1..16 (cells 3..18 of the array) -- the profile of the 1-D experiment along either axis, 0.5
    to 180.5 m2/s; the largest kick is sqrt(6 180.5 400) = 658 m, the largest drift 400 x 32 / 1000^2 = 0.013 cells"""
    if "basin" not in _MADE:
        size = BASIN + 4
        tm = np.zeros((size, size), dtype=np.int32)
        tm[2:-2, 2:-2] = 1
        d = np.full((size, size), MESH)
        still = np.zeros((size, size))
        prof = 1.0 + 0.9 * np.sin(2.0 * np.pi * (np.arange(size) - 1.5) / BASIN)
        kh = 50.0 * prof[:, None] * prof[None, :]
        kh[tm == 0] = np.nan
        _MADE["basin"] = ((2, BASIN + 3, 2, BASIN + 3), tm, d, d, still, still, kh)
    return _MADE["basin"]


def basin_release():
    """2^14 particles released uniformly over the wet cells"""
    rng = np.random.default_rng(6220)
    return 3.0 + BASIN * rng.random(WM_N), 3.0 + BASIN * rng.random(WM_N), np.zeros(WM_N, dtype=np.int32)


def marginal_errors(px, py, status):
    """the largest deviation of a column count and of a row count from N / 16, in multinomial standard errors
    sqrt(N p (1 - p)), p = 1 / 16; every particle must still be ACTIVE in the basin"""
    assert (status == 0).all()
    n, p = len(px), 1.0 / BASIN
    se = np.sqrt(n * p * (1.0 - p))
    cx = np.bincount(np.floor(px).astype(int) - 3, minlength=BASIN)
    cy = np.bincount(np.floor(py).astype(int) - 3, minlength=BASIN)
    assert len(cx) == BASIN and len(cy) == BASIN
    return float(np.abs(cx - n * p).max() / se), float(np.abs(cy - n * p).max() / se)
