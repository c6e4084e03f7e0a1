"""The rule of DESIGN.md section 6.19 restated twice for the tests, with no GPU and none of the library's code: a scalar loop
over the slots, and an array form (np.bincount for the counts, unbuffered np.add.at over the chunks and then over the cells
for the sums).  Both take the keys from tests/particle_order_numpy.py (section 6.18's rule, checked there).

The sum of a cell's run: the aligned groups of CHUNK consecutive slots are chunks; within a chunk the run's slots are added
one by one in ascending slot order, beginning with the first; the chunks' partials are added one by one in ascending chunk
order, beginning with the first."""
import numpy as np

import particle_order_numpy as PN

CHUNK = 64
SET, ADD = 0, 1


def slot_keys(box, px, py, status, perm):
    """(key of every slot, unordered): perm None is the identity; an index outside 0..n-1 is dead and sets the flag, as does a
    key below that of the slot before it"""
    n = len(px)
    ncells = PN.cells(box)[2]
    key = PN.keys(box, px, py, status)[0].astype(np.int64)
    if perm is None:
        perm = np.arange(n, dtype=np.int64)
    perm = np.asarray(perm, dtype=np.int64)
    ok = (perm >= 0) & (perm < n)
    skey = np.full(n, ncells, dtype=np.int64)
    skey[ok] = key[perm[ok]]
    return skey, int((not ok.all()) or bool((skey[1:] < skey[:-1]).any()))


def run_sum(slots, values, chunk=CHUNK):
    """the rule's sum of one run: slots ascending, values[k] the weight of slot k; chunk None: one sequential sum"""
    total = part = here = None
    for k in slots:
        g = k // chunk if chunk else 0
        if g != here:
            if part is not None:
                total = part if total is None else total + part
            part, here = float(values[k]), g
        else:
            part = part + float(values[k])
    return part if total is None else total + part


def sums_scalar(box, px, py, status, perm, weights):
    """(S, has, unordered) one slot at a time: S[a][c] the rule's sum of weights[a] (None: 1.0) in cell c, +0.0 where no
    live particle is; has[c]: the cell holds one"""
    n, ncells = len(px), PN.cells(box)[2]
    skey, unordered = slot_keys(box, px, py, status, perm)
    runs = {}
    for k in range(n):
        if skey[k] < ncells:
            runs.setdefault(int(skey[k]), []).append(k)
    S, has = np.zeros((len(weights), ncells)), np.zeros(ncells, dtype=bool)
    for a, w in enumerate(weights):
        sw = np.ones(n) if w is None else _by_slot(w, perm, n)
        for c, slots in runs.items():
            S[a, c] = run_sum(slots, sw)
            has[c] = True
    return S, has, unordered


def _by_slot(w, perm, n):
    if perm is None:
        return np.asarray(w)
    perm = np.asarray(perm, dtype=np.int64)
    ok = (perm >= 0) & (perm < n)
    out = np.zeros(n)
    out[ok] = np.asarray(w)[perm[ok]]
    return out


def sums_array(box, px, py, status, perm, weights):
    """the same by whole arrays, for keys in order: the (cell, chunk) groups are contiguous; a group's partial begins with its
    first slot and np.add.at adds the others in slot order; a cell's sum begins with its first partial and np.add.at adds
    the others in chunk order"""
    n, ncells = len(px), PN.cells(box)[2]
    skey, unordered = slot_keys(box, px, py, status, perm)
    live = np.flatnonzero(skey < ncells)
    cell = skey[live]
    count = np.bincount(cell, minlength=ncells)[:ncells] if ncells else np.zeros(0, dtype=np.int64)
    S, has = np.zeros((len(weights), ncells)), count > 0
    if len(live) == 0:
        return S, has, unordered
    group = cell * ((n + CHUNK - 1) // CHUNK + 1) + live // CHUNK
    first = np.ones(len(live), dtype=bool)
    first[1:] = group[1:] != group[:-1]
    gid = np.cumsum(first) - 1                                        # the group of every live slot
    gcell = cell[first]
    gfirst = np.ones(len(gcell), dtype=bool)
    gfirst[1:] = gcell[1:] != gcell[:-1]
    for a, w in enumerate(weights):
        if w is None:
            S[a] = count.astype(np.float64)
            continue
        v = _by_slot(w, perm, n)[live]
        part = v[first].copy()
        np.add.at(part, gid[~first], v[~first])
        S[a][gcell[gfirst]] = part[gfirst]
        np.add.at(S[a], gcell[~gfirst], part[~gfirst])
    return S, has, unordered


def apply(box, mode, alpha, S, has, fields):
    """the fields (ny x ld arrays, one per row of S) after the call, in place: SET stores alpha * S in every cell of the box,
    ADD adds alpha * S to the cells that hold a live particle"""
    xstart, xstop, ystart, ystop = box
    nxb, nyb, ncells = PN.cells(box)
    if ncells == 0:
        return
    for a, f in enumerate(fields):
        view = f[ystart - 1:ystop, xstart - 1:xstop]
        term = np.float64(alpha) * S[a].reshape(nyb, nxb)
        if mode == SET:
            view[...] = term
        else:
            m = has.reshape(nyb, nxb)
            view[m] = view[m] + term[m]


def same(a, b):
    """bit for bit"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))
