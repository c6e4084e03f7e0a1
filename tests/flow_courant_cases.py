"""Inputs the CPU and GPU tests of the flow step's stability check share: a plain and a special-value
case at tracer_cases' three shapes (260 x 12: three wave tiles with both seams in the box; 131 x 10: the odd pitch; 130 x 9
swept on a sub-box), the land overwrite of the invariance tests, and the restatement's record of each, made once and never
modified.  Nothing here needs a GPU.
"""
import math

import numpy as np

import flow_courant_numpy as FN
import tracer_cases as TC
from nemolite_boxes import SPECIAL, _host_inputs, host_grid

ARRAYS = ("dx_t", "dy_t", "un", "vn", "ht", "sshn_t")      # the C entry's order, after tmask
SHAPES = TC.SPECIAL_SHAPES
G = 9.80665
VISC = 100.0
RDT = 20.0                  # every number of the plain case below its default limit
RDT_BIG = 70.0              # the plain case's gravity-wave numbers on both sides of 1
LIMITS = FN.LIMITS
# at RDT_BIG the plain case's cells lie on both sides of each of these (test_flow_courant_numpy.py's census)
LIMITS_BIG = (1.0, 0.03, 0.014, 10.5)
PATCH = TC.PATCH            # rows 3..6, columns 8..39 (0-based), all wet but one open cell: the extremes and their ties
_MADE = {}


def _metrics_and_flow(rng, tm):
    Gd = host_grid(rng, tm)                                 # dx_t, dy_t: 900 .. 1100 in wet cells, 0 elsewhere
    H = _host_inputs(rng, tm.shape)
    return {"dx_t": Gd["dx_t"], "dy_t": Gd["dy_t"], **{k: H[k] for k in ("un", "vn", "ht", "sshn_t")}}


def plain_host(ld, ny):
    """(tm, A): random_mask, non-uniform metrics, velocities with signed zeros"""
    key = ("plain", ld, ny)
    if key not in _MADE:
        rng = np.random.default_rng(ld * 7 + ny)
        tm = TC.random_mask(rng, ny, ld)
        _MADE[key] = (tm, _metrics_and_flow(rng, tm))
    return _MADE[key]


def _sprinkle(rng, a, share):
    pick = rng.random(a.shape) < share
    a[pick] = rng.choice(SPECIAL, size=int(pick.sum()))


def special_host(ld, ny):
    """(tm, A) for arrays of at least 9 rows and 42 columns: the plain inputs, then
      * nemolite_boxes.SPECIAL (subnormals, signed zeros, infinities, NaN of both signs, 1e300, 1e154) in 2 % of un and vn, in
        0.5 % of ht and sshn_t and in 0.4 % of dx_t and dy_t;
      * sshn_t = -ht (d == 0) on 1 % of the wet cells and sshn_t = -2 ht (d < 0) on another 1 %;
      * PATCH, all wet, with dx_t = dy_t = 500 (the smallest spacing: the largest k2), ht = 1e300, sshn_t = 0 (the deepest
        column) and velocities from tracer_cases.PATCH_VELOCITIES: the gravity-wave and the viscous maximum are attained in
        every sound cell of the patch, so the record must name the lowest index; two cells with d = 5e-324, the smallest
        column there is, twice;
      * whatever the random picks hit, in PATCH: cells with d < 0, d == 0 and a NaN d, a cell with dx_t == 0, an open cell (tmask < 0) with an
        infinite un on the face towards its wet western neighbour, and a NaN in vn."""
    key = ("special", ld, ny)
    if key in _MADE:
        return _MADE[key]
    rng = np.random.default_rng(ld * 7 + ny + 1000)
    tm = TC.random_mask(rng, ny, ld)
    A = _metrics_and_flow(rng, tm)
    for k in ("un", "vn"):
        _sprinkle(rng, A[k], 0.02)
    for k in ("ht", "sshn_t"):
        _sprinkle(rng, A[k], 0.005)
    for k in ("dx_t", "dy_t"):
        _sprinkle(rng, A[k], 0.004)
    pick = rng.random(tm.shape)
    zero, neg = (pick < 0.01) & (tm > 0), (pick >= 0.01) & (pick < 0.02) & (tm > 0)
    A["sshn_t"][zero] = -A["ht"][zero]
    A["sshn_t"][neg] = -2.0 * A["ht"][neg]
    rows, cols = PATCH
    tm[PATCH] = 1
    A["dx_t"][PATCH] = A["dy_t"][PATCH] = 500.0
    A["ht"][PATCH], A["sshn_t"][PATCH] = 1.0e300, 0.0
    for k in ("un", "vn"):
        A[k][PATCH] = rng.choice(TC.PATCH_VELOCITIES, size=A[k][PATCH].shape)
    j0, i0 = rows.start, cols.start
    A["ht"][j0 + 1, i0 + 3] = A["ht"][j0 + 2, i0 + 5] = 5.0e-324
    A["ht"][j0 + 1:j0 + 3, i0 + 31] = 12.0
    A["sshn_t"][j0 + 2, i0 + 31] = -13.0                    # d < 0
    A["sshn_t"][j0 + 1, i0 + 31] = -12.0                    # d == 0
    A["ht"][j0 + 3, i0 + 31] = np.nan                       # d is a NaN
    A["dx_t"][j0, i0 + 31] = 0.0                            # an infinite ix
    tm[j0 + 3, i0 + 2] = -1                                 # an open cell ...
    A["un"][j0 + 3, i0 + 1] = np.inf                        # ... and an infinite velocity on its western face
    A["vn"][j0 + 1, i0 + 20] = np.nan
    _MADE[key] = (tm, A)
    return _MADE[key]


def host(kind, ld, ny):
    return plain_host(ld, ny) if kind == "plain" else special_host(ld, ny)


def arrays(A):
    return [A[k] for k in ARRAYS]


def reference(kind, ld, ny, box, rdt, limits=LIMITS, visc=VISC):
    """the array restatement's record of the case; made once"""
    key = (kind, ld, ny, tuple(box), float(rdt), tuple(limits), float(visc))
    if key not in _MADE:
        tm, A = host(kind, ld, ny)
        _MADE[key] = FN.flow_courant(rdt, G, visc, box, tm, *arrays(A), *limits)
    return _MADE[key]


def land_overwritten(tm, A):
    """a copy with NaN in un / vn on every face that touches land (tracer_cases.land_faces) and NaN, an infinity, a negative
    number and 0 in ht, sshn_t, dx_t, dy_t of every land cell"""
    fu, fv = TC.land_faces(tm)
    A2 = {k: v.copy() for k, v in A.items()}
    A2["un"][fu] = np.nan
    A2["vn"][fv] = np.nan
    for k, fill in (("ht", np.nan), ("sshn_t", -np.inf), ("dx_t", -3.0), ("dy_t", np.nan)):
        A2[k][tm == 0] = fill
    return A2


def at_the_limits(rec):
    """(limits at which the cells holding each extreme count, limits one ulp beyond, at which no cell does)"""
    up = [float(np.nextafter(x, math.inf)) for x in rec[:3]]
    return tuple(rec[:4]), (*up, float(np.nextafter(rec.depth_min, -math.inf)))
