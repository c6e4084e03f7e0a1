"""Two independent CPU restatements of the particle release.

release_scalar walks the candidates one at a time through the rule as it is written, with Philox4x32-10 in Python integers and
one cursor over the slots; release_vector makes every candidate at once with Philox in uint64 arrays, flatnonzero and cumsum,
and never loops over a candidate or a slot.  Both work in place and return the record.

A source table is an int64 array of nsources x 8: x, y, rx, ry as the bits of doubles, next_id, count, tag, pad.  The record is
an int32 array of 16: requested (two words, low first), released, foreign, on_land, dropped, edge, nfree, clamped, bad_source
and six zeros.  box = (xstart, xstop, ystart, ystop), 1-based and local; off = (offx, offy), global minus local; tm: the mask,
tm[j - 1, i - 1] is cell (i, j); born_value: tick + *tick_dev; tag and born may be None.
"""
import math

import numpy as np

import dispersal_numpy as PN
import drifter_numpy as DN

ACTIVE, LEFT, OPEN, GROUNDED, FREE = range(5)
F = np.float64
RECORD = 16
REQUESTED, RELEASED, FOREIGN, ON_LAND, DROPPED, EDGE, NFREE, CLAMPED, BAD_SOURCE = 0, 2, 3, 4, 5, 6, 7, 8, 9
X, Y, RX, RY, NEXT_ID, COUNT, TAG, PAD = range(8)
MASK32, MASK64 = PN.MASK32, PN.MASK64
CHUNK, TILE, SCAN_TILE = 256, 4096, 2048          # the plan's constants


def table(x, y, rx, ry, next_id, count, tag=None):
    """a host source table from sequences of one length"""
    ns = len(x)
    t = np.zeros((ns, 8), dtype=np.int64)
    for k, c in enumerate((x, y, rx, ry)):
        t[:, k] = np.asarray(c, dtype=np.float64).view(np.int64)
    t[:, NEXT_ID] = np.asarray([_signed(int(v)) for v in next_id], dtype=np.int64)
    t[:, COUNT] = np.asarray(count, dtype=np.int64)
    t[:, TAG] = np.arange(ns) * 7 + 3 if tag is None else np.asarray(tag, dtype=np.int64)
    return t


def _signed(v):
    v &= MASK64
    return v - (1 << 64) if v >> 63 else v


def record(requested, released, foreign, on_land, dropped, edge, nfree, clamped, bad):
    r = np.zeros(RECORD, dtype=np.int32)
    r[:2] = np.array([requested], dtype=np.int64).view(np.int32)
    r[2:10] = released, foreign, on_land, dropped, edge, nfree, clamped, bad
    return r


def requested(rec):
    return int(rec[:2].view(np.int64)[0])


def invariant(rec):
    return requested(rec) == int(rec[RELEASED]) + int(rec[DROPPED]) + int(rec[FOREIGN]) + int(rec[ON_LAND])


# ---------------------------------------------------------------------------------------------- one candidate at a time
def release_scalar(box, off, tm, sources, max_count, seed, born_value, px, py, status, ids, tag=None, born=None):
    xs, xe, ys, ye = box
    ox, oy = off
    key = PN._key(seed)
    st = status.tolist()
    n, p = len(st), 0
    req = rel = foreign = land = dropped = edge = clamped = bad = 0
    given = []
    with np.errstate(over="ignore", invalid="ignore"):
        for s in range(len(sources)):
            x, y, rx, ry = (F(v) for v in sources[s, :4].view(np.float64))
            count, first = int(sources[s, COUNT]), int(sources[s, NEXT_ID])
            if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(rx) and np.isfinite(ry) and rx >= 0 and ry >= 0
                    and count >= 0):
                bad += 1
                given.append(0)
                continue
            c = min(count, max_count)
            clamped += count > max_count
            req += c
            given.append(c)
            for m in range(c):
                ident = (first + m) & MASK64
                w = PN.philox((ident & MASK32, 1, ident >> 32, 0), key)
                gx, gy = x + rx * PN.sym(w[0]), y + ry * PN.sym(w[1])
                if not (np.isfinite(gx) and np.isfinite(gy) and F(xs + ox) <= gx < F(xe + 1 + ox)
                        and F(ys + oy) <= gy < F(ye + 1 + oy)):
                    foreign += 1
                    continue
                lx, ly = gx - F(ox), gy - F(oy)
                if not DN.inbox(box, lx, ly):
                    new, edge = LEFT, edge + 1
                elif tm[int(math.floor(ly)) - 1, int(math.floor(lx)) - 1] == 0:
                    land += 1
                    continue
                else:
                    new = ACTIVE
                while p < n and st[p] != FREE:
                    p += 1
                if p == n:
                    dropped += 1
                    continue
                px[p], py[p], status[p], ids[p] = lx, ly, new, _signed(ident)
                if tag is not None:
                    tag[p] = sources[s, TAG]
                if born is not None:
                    born[p] = born_value
                rel += 1
                p += 1
    for s, c in enumerate(given):
        sources[s, NEXT_ID] = _signed(int(sources[s, NEXT_ID]) + c)
    return record(req, rel, foreign, land, dropped, edge, int(np.count_nonzero(status == FREE)), clamped, bad)


# ---------------------------------------------------------------------------------------------- all candidates at once
def candidates(sources, max_count, seed):
    """every candidate of a call, source-major: (source, id as uint64, gx, gy), the given counts c_s and (clamped, bad)"""
    v = sources[:, :4].view(np.float64)
    count = sources[:, COUNT]
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(v).all(axis=1) & (v[:, RX] >= 0) & (v[:, RY] >= 0) & (count >= 0)
    c = np.where(valid, np.minimum(count, max_count), 0)
    src = np.repeat(np.arange(len(sources)), c)
    m = np.arange(len(src)) - np.repeat(np.cumsum(c) - c, c)
    ident = sources[src, NEXT_ID].astype(np.uint64) + m.astype(np.uint64)                 # wraps
    k0, k1 = PN._key(seed)
    w = PN.philox_v(ident & np.uint64(MASK32), np.uint64(1), ident >> np.uint64(32), np.uint64(0), k0, k1)
    with np.errstate(over="ignore", invalid="ignore"):
        gx = v[src, X] + v[src, RX] * PN.sym_v(w[0])
        gy = v[src, Y] + v[src, RY] * PN.sym_v(w[1])
    return src, ident, gx, gy, c, (int(np.count_nonzero(valid & (count > max_count))), int(np.count_nonzero(~valid)))


def release_vector(box, off, tm, sources, max_count, seed, born_value, px, py, status, ids, tag=None, born=None):
    xs, xe, ys, ye = box
    ox, oy = off
    src, ident, gx, gy, c, (clamped, bad) = candidates(sources, max_count, seed)
    with np.errstate(invalid="ignore"):
        owned = (np.isfinite(gx) & np.isfinite(gy) & (gx >= float(xs + ox)) & (gx < float(xe + 1 + ox))
                 & (gy >= float(ys + oy)) & (gy < float(ye + 1 + oy)))
        lx, ly = gx - float(ox), gy - float(oy)
    inb = owned & DN._inbox_v(box, lx, ly)
    J = np.where(inb, np.floor(np.where(inb, ly, 1.0)), 1).astype(np.int64) - 1
    I = np.where(inb, np.floor(np.where(inb, lx, 1.0)), 1).astype(np.int64) - 1
    wet = inb & (tm[J, I] != 0) if len(src) else inb
    leaves = owned & ~inb
    acc = np.flatnonzero(wet | leaves)
    slots = np.flatnonzero(status == FREE)
    k = min(len(acc), len(slots))
    a, p = acc[:k], slots[:k]
    px[p], py[p], status[p] = lx[a], ly[a], np.where(leaves[a], LEFT, ACTIVE)
    ids[p] = ident[a].view(np.int64)
    if tag is not None:
        tag[p] = sources[src[a], TAG]
    if born is not None:
        born[p] = born_value
    sources[:, NEXT_ID] = (sources[:, NEXT_ID].astype(np.uint64) + c.astype(np.uint64)).view(np.int64)
    return record(int(c.sum()), k, int(np.count_nonzero(~owned)), int(np.count_nonzero(inb & ~wet)), len(acc) - k,
                  int(np.count_nonzero(leaves)), len(slots) - k, clamped, bad)
