"""Inputs the CPU and GPU tests of the particle order share, made once and never modified.  Nothing
here needs a GPU.

A case is (distribution, box, n).  The counts straddle a wave (64), a block's step (256) and a block's keys (TILE, read from
the kernel's source) and reach four blocks with a ragged last one and 70001; the boxes are an empty one, one cell, 15 x 16
(240 cells: one radix pass), 16 x 16 (the dead key 256 needs a second), 255 x 257 (the dead key 65535 still fits two), 256 x
256 (a third), 4096 x 4096 (the dead key 2^24 needs the fourth) and 5000 x 5000, all but one offset from (1, 1)."""
import os
import re

import numpy as np

import particle_order_numpy as PN

_SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "dl_esm_inf_amd", "csrc", "dlesm_particle_sort.hip")
TILE = int(re.search(r"constexpr int SORT_TILE = (\d+);", open(_SRC).read()).group(1))
NS = [1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 517, 70001]
BOXES = {
    "empty": (5, 4, 3, 10),
    "1x1": (7, 7, 9, 9),
    "15x16": (3, 17, 5, 20),
    "16x16": (3, 18, 5, 20),
    "255x257": (2, 256, 4, 260),
    "256x256": (1, 256, 1, 256),
    "4096x4096": (3, 4098, 2, 4097),
    "5000x5000": (2, 5001, 7, 5006),
}
PASSES = {"empty": 0, "1x1": 1, "15x16": 1, "16x16": 2, "255x257": 2, "256x256": 3, "4096x4096": 4, "5000x5000": 4}
DISTS = ["uniform", "onecell", "twocells", "sorted", "reverse", "alldead", "alllive", "mixed", "specials"]
_MADE = {}


def _inside(rng, box, n):
    xstart, xstop, ystart, ystop = box
    nxb, nyb = max(xstop - xstart + 1, 1), max(ystop - ystart + 1, 1)
    # a cell and a fraction below one: never on the far edge, whatever the rounding
    x = xstart + rng.integers(0, nxb, n) + rng.integers(0, 1024, n) / 1024.0
    y = ystart + rng.integers(0, nyb, n) + rng.integers(0, 1024, n) / 1024.0
    return x, y


def _seed(dist, box, n):
    rng_key = (DISTS.index(dist),) + tuple(box) + (n,)
    return int(np.dot(rng_key, [1000003, 10007, 1009, 101, 11, 1])) % 2 ** 32


def _make(dist, box, n):
    xstart, xstop, ystart, ystop = box
    nxb, nyb = max(xstop - xstart + 1, 1), max(ystop - ystart + 1, 1)
    rng = np.random.default_rng(_seed(dist, box, n))
    st = np.zeros(n, dtype=np.int32)
    if dist in ("uniform", "mixed", "specials"):
        # a region a quarter of the box wider than the box on every side
        x = xstart - 0.25 * nxb - 1.0 + (1.5 * nxb + 2.0) * rng.random(n)
        y = ystart - 0.25 * nyb - 1.0 + (1.5 * nyb + 2.0) * rng.random(n)
        if dist == "mixed":
            st = rng.choice(np.array([0, 0, 0, 1, 2, 3, 7, -1], dtype=np.int32), n)
        if dist == "specials":
            bad = np.array([np.nan, np.inf, -np.inf, -np.nan])
            hit = rng.random(n) < 0.2
            x = np.where(hit, bad[rng.integers(0, 4, n)], x)
            hit = rng.random(n) < 0.2
            y = np.where(hit, bad[rng.integers(0, 4, n)], y)
    elif dist == "onecell":
        x = np.full(n, xstart + nxb // 2) + rng.integers(0, 1024, n) / 1024.0
        y = np.full(n, ystart + nyb // 2) + rng.integers(0, 1024, n) / 1024.0
    elif dist == "twocells":
        # the later cell first, so that every second particle has to pass every first
        odd = np.arange(n) % 2 == 1
        x = np.where(odd, float(xstart), float(xstop if xstop >= xstart else xstart)) + 0.5
        y = np.where(odd, float(ystart), float(ystop if ystop >= ystart else ystart)) + 0.25
    else:
        x, y = _inside(rng, box, n)
        if dist in ("sorted", "reverse"):
            key = (np.floor(y).astype(np.int64) - ystart) * nxb + (np.floor(x).astype(np.int64) - xstart)
            o = np.argsort(key, kind="stable")
            o = o[::-1] if dist == "reverse" else o
            x, y = x[o], y[o]
        if dist == "alldead":
            st = rng.integers(1, 4, n).astype(np.int32)
    return np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64), st


def case(dist, boxname, n):
    """(px, py, status) of a case"""
    key = ("case", dist, boxname, n)
    if key not in _MADE:
        _MADE[key] = _make(dist, BOXES[boxname], n)
        for a in _MADE[key]:
            a.setflags(write=False)
    return _MADE[key]


def reference(dist, boxname, n):
    """(perm, nlive) of a case by the array restatement; made once"""
    key = ("ref", dist, boxname, n)
    if key not in _MADE:
        perm, nlive = PN.order(BOXES[boxname], *case(dist, boxname, n))
        perm.setflags(write=False)
        _MADE[key] = (perm, nlive)
    return _MADE[key]


def edge_particles(box):
    """(px, py, status, live) on and next to the edges of a box"""
    xstart, xstop, ystart, ystop = box
    xm, ym = xstart + 0.5, ystart + 0.5
    rows = [
        (float(xstart), ym, True), (xm, float(ystart), True),                                  # the first coordinate is in
        (float(np.nextafter(xstop + 1.0, 0.0)), ym, True), (xm, float(np.nextafter(ystop + 1.0, 0.0)), True),
        (float(xstop + 1), ym, False), (xm, float(ystop + 1), False),                          # the far edge is out
        (float(np.nextafter(float(xstart), 0.0)), ym, False), (xm, float(np.nextafter(float(ystart), 0.0)), False),
        (float("nan"), ym, False), (xm, float("nan"), False), (float("inf"), ym, False), (xm, float("inf"), False),
        (float("-inf"), ym, False), (xm, float("-inf"), False), (float("nan"), float("inf"), False),
    ]
    px, py = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    return px, py, np.zeros(len(rows), dtype=np.int32), np.array([r[2] for r in rows])
