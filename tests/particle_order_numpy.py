"""The rule of DESIGN.md section 6.18 restated twice for the tests, with no GPU and none of the library's code: the key rule
in whole arrays followed by numpy's stable argsort, and a scalar loop that drops the particles into one bucket per key."""
import math

import numpy as np

ACTIVE = 0


def cells(box):
    xstart, xstop, ystart, ystop = box
    nxb, nyb = xstop - xstart + 1, ystop - ystart + 1
    return (nxb, nyb, nxb * nyb) if nxb > 0 and nyb > 0 else (max(nxb, 0), max(nyb, 0), 0)


def passes(box):
    """the radix passes a box costs: ceil(bit_length(ncells) / 8)"""
    return (int(cells(box)[2]).bit_length() + 7) // 8


def keys(box, px, py, status):
    """(key, live): unsigned 32-bit keys; inbox is evaluated in double before any conversion"""
    xstart, xstop, ystart, ystop = box
    nxb, _, ncells = cells(box)
    with np.errstate(invalid="ignore"):
        live = (status == ACTIVE) & (px >= xstart) & (px < xstop + 1.0) & (py >= ystart) & (py < ystop + 1.0)
    key = np.full(px.shape, ncells, dtype=np.int64)
    i, j = np.floor(px[live]).astype(np.int64), np.floor(py[live]).astype(np.int64)
    key[live] = (j - ystart) * nxb + (i - xstart)
    assert key.min(initial=0) >= 0 and key.max(initial=0) <= 2 ** 32 - 2
    return key.astype(np.uint32), live


def order(box, px, py, status):
    """(perm, nlive) by the array form"""
    key, live = keys(box, px, py, status)
    return np.argsort(key, kind="stable").astype(np.int32), int(live.sum())


def order_scalar(box, px, py, status):
    """(perm, nlive) one particle at a time: a bucket per key, filled in index order, emptied in key order"""
    xstart, xstop, ystart, ystop = box
    nxb, _, ncells = cells(box)
    buckets, dead = {}, []
    for p in range(len(px)):
        x, y = float(px[p]), float(py[p])
        if int(status[p]) == ACTIVE and xstart <= x < xstop + 1.0 and ystart <= y < ystop + 1.0:
            buckets.setdefault((math.floor(y) - ystart) * nxb + (math.floor(x) - xstart), []).append(p)
        else:
            dead.append(p)
    perm = [p for k in sorted(buckets) for p in buckets[k]]
    assert all(0 <= k < ncells for k in buckets)
    return np.array(perm + dead, dtype=np.int32), len(perm)


def permute(perm, src, dst):
    """dst[k] = src[perm[k]]; an index outside 0..n-1 leaves dst[k] alone"""
    n = len(perm)
    ok = (perm >= 0) & (perm < n)
    dst[:n][ok] = src[perm[ok]]
