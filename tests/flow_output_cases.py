"""Inputs the CPU and GPU tests of the model's output fields share: a plain and a special-value case
at tracer_cases' three shapes (260 x 12: three wave tiles with both seams in the box; 131 x 10: the odd pitch; 130 x 9 swept
on the sub-box (5, 100, 3, 8)), on the masks of flow_courant_cases (the same seeds, the mask drawn first), the land overwrite
of the invariance tests, and the restatement's arrays of each, made once and never modified.  Nothing here needs a GPU.
"""
import numpy as np

import flow_output_numpy as ON
import tracer_cases as TC
from nemolite_boxes import SPECIAL, _host_inputs

ARRAYS = ("dx_v", "dy_u", "un", "vn", "ht", "sshn_t")      # the C entry's order, after tmask
SHAPES = TC.SPECIAL_SHAPES
SENTINEL = -7.0
WEIGHT = 0.375              # of the ADD runs: twice into the same arrays
PATCH = TC.PATCH            # rows 3..6, columns 8..39 (0-based), all wet but one open pair in the special case
ALL = tuple(range(ON.COUNT))
SELECTIONS = [ALL] + [(k,) for k in ALL] + [(ON.UT, ON.VT, ON.SPEED)]
_MADE = {}


def _fields(rng, tm):
    """dx_v, dy_u: 900 .. 1100 everywhere, non-uniform; velocities with signed zeros"""
    H = _host_inputs(rng, tm.shape)
    A = {"dx_v": 900.0 + 200.0 * rng.random(tm.shape), "dy_u": 900.0 + 200.0 * rng.random(tm.shape)}
    A.update({k: H[k] for k in ("un", "vn", "ht", "sshn_t")})
    return A


def plain_host(ld, ny):
    key = ("plain", ld, ny)
    if key not in _MADE:
        rng = np.random.default_rng(ld * 7 + ny)
        tm = TC.random_mask(rng, ny, ld)
        _MADE[key] = (tm, _fields(rng, tm))
    return _MADE[key]


def _sprinkle(rng, a, share):
    pick = rng.random(a.shape) < share
    a[pick] = rng.choice(SPECIAL, size=int(pick.sum()))


def special_host(ld, ny):
    """(tm, A) for arrays of at least 9 rows and 42 columns: the plain kind of inputs, then
      * nemolite_boxes.SPECIAL (subnormals, signed zeros, infinities, NaN of both signs, 1e300, 1e154) in 2 % of un and vn, in
        0.5 % of ht and sshn_t and in 0.4 % of dx_v and dy_u -- a metric of 0 next to one of -0.0 divides by zero;
      * sshn_t = -ht (d == 0) on 1 % of the wet cells;
      * PATCH, all wet, velocities from tracer_cases.PATCH_VELOCITIES; in it, whatever the random picks hit: an open cell
        (tmask < 0) with an open cell east of it and infinite / 1e300 velocities on the faces between and around them (read as
        they are), ut*ut that overflows, a NaN in vn, dx_v == 0 twice side by side (an infinite dvdx, or 0/0), a NaN ht."""
    key = ("special", ld, ny)
    if key in _MADE:
        return _MADE[key]
    rng = np.random.default_rng(ld * 7 + ny + 1000)
    tm = TC.random_mask(rng, ny, ld)
    A = _fields(rng, tm)
    for k in ("un", "vn"):
        _sprinkle(rng, A[k], 0.02)
    for k in ("ht", "sshn_t"):
        _sprinkle(rng, A[k], 0.005)
    for k in ("dx_v", "dy_u"):
        _sprinkle(rng, A[k], 0.004)
    pick = rng.random(tm.shape)
    zero = (pick < 0.01) & (tm > 0)
    A["sshn_t"][zero] = -A["ht"][zero]
    rows, cols = PATCH
    tm[PATCH] = 1
    for k in ("un", "vn"):
        A[k][PATCH] = rng.choice(TC.PATCH_VELOCITIES, size=A[k][PATCH].shape)
    j0, i0 = rows.start, cols.start
    tm[j0 + 3, i0 + 2] = -1                                 # the open cell of flow_courant_cases ...
    A["un"][j0 + 3, i0 + 1] = np.inf                        # ... with an infinite velocity on its western face
    A["un"][j0 + 2, i0 + 6] = 1.0e300                       # ut*ut overflows
    A["vn"][j0 + 1, i0 + 20] = np.nan
    A["dx_v"][j0 + 1, i0 + 12] = A["dx_v"][j0 + 1, i0 + 13] = 0.0
    A["ht"][j0 + 2, i0 + 25] = np.nan
    _MADE[key] = (tm, A)
    return _MADE[key]


def host(kind, ld, ny):
    return plain_host(ld, ny) if kind == "plain" else special_host(ld, ny)


def outputs(shape, sel):
    """sentinel-filled arrays for the selected outputs, None for the others"""
    return [np.full(shape, SENTINEL) if k in sel else None for k in range(ON.COUNT)]


def inputs_for(A, sel, fill=None):
    """the six inputs in ARRAYS' order; one no output of `sel` reads is None, or an all-NaN array with fill = 'nan'"""
    need = ON.needs([0 if k in sel else None for k in range(ON.COUNT)])
    return [A[n] if need[m] else (None if fill is None else np.full(A[n].shape, np.nan)) for m, n in enumerate(ARRAYS)]


def reference(kind, ld, ny, box, mode, sel=ALL):
    """what the array restatement leaves in sentinel-filled outputs: one SET call, or two ADD calls with WEIGHT; made once"""
    key = (kind, ld, ny, tuple(box), mode, tuple(sel))
    if key not in _MADE:
        tm, A = host(kind, ld, ny)
        out = outputs(tm.shape, sel)
        for _ in range(2 if mode == ON.ADD else 1):
            ON.flow_output(mode, WEIGHT, box, tm, *inputs_for(A, sel), out)
        _MADE[key] = out
    return _MADE[key]


def land_overwritten(tm, A):
    """a copy with NaN in un / vn on every face that touches land (tracer_cases.land_faces) and NaN, an infinity and -3 in ht,
    sshn_t, dx_v, dy_u of every land cell"""
    fu, fv = TC.land_faces(tm)
    A2 = {k: v.copy() for k, v in A.items()}
    A2["un"][fu] = np.nan
    A2["vn"][fv] = np.nan
    for k, fill in (("ht", np.nan), ("sshn_t", -np.inf), ("dx_v", -3.0), ("dy_u", np.nan)):
        A2[k][tm == 0] = fill
    return A2


def census(tm, box):
    """(wet, corner true, corner false, land to the west, corner true with an open cell east and north-east) over the box"""
    S = ON._view(box)
    wet = S(tm) > 0
    corner = ON.corner_of(tm, box)
    open_pair = wet & corner & (S(tm, 1, 0) < 0) & (S(tm, 1, 1) < 0)
    return (int(wet.sum()), int((wet & corner).sum()), int((wet & ~corner).sum()), int((wet & (S(tm, -1, 0) == 0)).sum()),
            int(open_pair.sum()))
