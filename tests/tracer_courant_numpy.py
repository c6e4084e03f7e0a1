"""Independent CPU evaluation of the tracer schemes' Courant check of DESIGN.md section 6.14.

TEST INFRASTRUCTURE.  The reference holds no such diagnostic, so its specification is frozen in DESIGN.md section 6.14 and
nothing in the reference can pin it.  Two evaluations are written here from that text, separately:
  * whole-array numpy expressions (`tracer_courant`): the face numbers from tracer_hancock_numpy.courant (and through it
    `weights`), the switches, the outflow number and the record's members over shifted views of the box;
  * a plain scalar loop (`tracer_courant_scalar`), one cell at a time, line by line, that evaluates w only in the cell and
    its four neighbours and keeps the running maxima with their first (= lowest) index.
Both round every operation in double precision in the association order the parentheses give and choose with selects.  Every
member of the record is a maximum, an integer or a lowest index, so the two are required to agree with each other, and with
the GPU, in every member exactly -- the two maxima by value (the sign of a zero is unspecified).

Index convention and arguments: tests/tracer_numpy.py; the box is 1-based inclusive with a one-cell ring inside the array.
"""
import collections
import math

import numpy as np

from tracer_hancock_numpy import courant, weights
from tracer_numpy import _div, _view

DBL_MAX = float(np.finfo(np.float64).max)
Record = collections.namedtuple(
    "Record", "face_max outflow_max face_index outflow_index face_over outflow_over invalid wet")
EMPTY = Record(0.0, 0.0, -1, -1, 0, 0, 0, 0)


def _valid(x):
    with np.errstate(all="ignore"):
        return (x >= 0.0) & (x <= DBL_MAX)


def cells(rdt, box, tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v):
    """(wet, m, has_m, o, has_o, bad) over the box: per-cell values of section 6.14 (m is -1.0 where there is none)"""
    S = _view(box)
    T = tmask
    wet = S(T) > 0
    on = [S(T, 1, 0) != 0, S(T, -1, 0) != 0, S(T, 0, 1) != 0, S(T, 0, -1) != 0]
    n = courant(rdt, box, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v)
    w = S(weights(rdt, area_t, ht, sshn_t))
    with np.errstate(all="ignore"):
        r1 = (S(sshn_u) + S(hu)) * S(un)
        r2 = (S(sshn_u, -1, 0) + S(hu, -1, 0)) * S(un, -1, 0)
        r3 = (S(sshn_v) + S(hv)) * S(vn)
        r4 = (S(sshn_v, 0, -1) + S(hv, 0, -1)) * S(vn, 0, -1)
        o1 = np.where(on[0] & (r1 > 0.0), r1, 0.0)
        o2 = np.where(on[1] & (r2 < 0.0), -r2, 0.0)
        o3 = np.where(on[2] & (r3 > 0.0), r3, 0.0)
        o4 = np.where(on[3] & (r4 < 0.0), -r4, 0.0)
        o = (((o1 + o2) + o3) + o4) * w
        m = np.full(wet.shape, -1.0)
        bad = ~((w > 0.0) & (w <= DBL_MAX))
        for k in range(4):
            ok = on[k] & _valid(n[k])
            m = np.where(ok & (n[k] > m), n[k], m)
            bad = bad | (on[k] & ~_valid(n[k]))
        bad = bad | ~_valid(o)
    return wet, m, wet & (m >= 0.0), o, wet & _valid(o), wet & bad


def tracer_courant(rdt, box, tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, face_limit=0.5, outflow_limit=1.0):
    """DESIGN.md section 6.14 on whole arrays; the argument order of dlesm_tracer_courant_f64"""
    xs, xe, ys, ye = box
    if xe < xs or ye < ys:
        return EMPTY
    ny, ld = tmask.shape
    assert xs >= 2 and ys >= 2 and xe <= ld - 1 and ye <= ny - 1                      # the ring: no view wraps
    wet, m, has_m, o, has_o, bad = cells(rdt, box, tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v)
    jj, ii = np.mgrid[ys - 1:ye, xs - 1:xe]
    index = jj.astype(np.int64) * ld + ii

    def top(x, has):
        if not has.any():
            return 0.0, -1
        best = x[has].max()
        return float(best), int(index[has & (x == best)].min())
    face_max, face_index = top(m, has_m)
    outflow_max, outflow_index = top(o, has_o)
    return Record(face_max, outflow_max, face_index, outflow_index, int((has_m & (m >= face_limit)).sum()),
                  int((has_o & (o >= outflow_limit)).sum()), int(bad.sum()), int(wet.sum()))


def _valid_scalar(x):
    return x >= 0.0 and x <= DBL_MAX


def tracer_courant_scalar(rdt, box, tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, face_limit=0.5,
                          outflow_limit=1.0):
    """the same rule, one cell at a time; i, j are 0-based here"""
    xs, xe, ys, ye = box
    rdt = float(rdt)
    ny, ld = tmask.shape

    def w(i, j):
        assert 0 <= i < ld and 0 <= j < ny
        with np.errstate(all="ignore"):
            return _div(rdt, np.float64(area_t[j, i]) * (np.float64(ht[j, i]) + np.float64(sshn_t[j, i])))

    face_max = outflow_max = None
    face_index = outflow_index = -1
    face_over = outflow_over = invalid = wet = 0
    for j in range(ys - 1, ye):
        for i in range(xs - 1, xe):
            if tmask[j, i] <= 0:
                continue
            assert 1 <= i <= ld - 2 and 1 <= j <= ny - 2          # the ring
            wet += 1
            r1 = (float(sshn_u[j, i]) + float(hu[j, i])) * float(un[j, i])
            r2 = (float(sshn_u[j, i - 1]) + float(hu[j, i - 1])) * float(un[j, i - 1])
            r3 = (float(sshn_v[j, i]) + float(hv[j, i])) * float(vn[j, i])
            r4 = (float(sshn_v[j - 1, i]) + float(hv[j - 1, i])) * float(vn[j - 1, i])
            on1, on2 = tmask[j, i + 1] != 0, tmask[j, i - 1] != 0
            on3, on4 = tmask[j + 1, i] != 0, tmask[j - 1, i] != 0
            here = w(i, j)
            n1 = abs(r1) * (here if r1 >= 0.0 else w(i + 1, j))
            n2 = abs(r2) * (w(i - 1, j) if r2 >= 0.0 else here)
            n3 = abs(r3) * (here if r3 >= 0.0 else w(i, j + 1))
            n4 = abs(r4) * (w(i, j - 1) if r4 >= 0.0 else here)
            o1 = r1 if on1 and r1 > 0.0 else 0.0
            o2 = -r2 if on2 and r2 < 0.0 else 0.0
            o3 = r3 if on3 and r3 > 0.0 else 0.0
            o4 = -r4 if on4 and r4 < 0.0 else 0.0
            o = (((o1 + o2) + o3) + o4) * here
            m = None
            bad = not (here > 0.0 and here <= DBL_MAX)
            for on, n in ((on1, n1), (on2, n2), (on3, n3), (on4, n4)):
                if not on:
                    continue
                if not _valid_scalar(n):
                    bad = True
                elif m is None or n > m:
                    m = n
            if not _valid_scalar(o):
                bad = True
            invalid += bad
            at = j * ld + i
            if m is not None:
                if face_max is None or m > face_max:              # cells come in index order: the first one stays
                    face_max, face_index = m, at
                face_over += m >= face_limit
            if _valid_scalar(o):
                if outflow_max is None or o > outflow_max:
                    outflow_max, outflow_index = o, at
                outflow_over += o >= outflow_limit
    return Record(0.0 if face_max is None else face_max, 0.0 if outflow_max is None else outflow_max, face_index,
                  outflow_index, int(face_over), int(outflow_over), int(invalid), wet)


def same_record(a, b):
    """every member equal: the maxima by value, the integers exactly"""
    a, b = Record(*a), Record(*b)
    return (not math.isnan(a.face_max) and not math.isnan(a.outflow_max) and a.face_max == b.face_max
            and a.outflow_max == b.outflow_max and tuple(int(x) for x in a[2:]) == tuple(int(x) for x in b[2:]))


def rdt_limit(rdt, rec, face_limit=0.5, outflow_limit=1.0):
    """the estimate psy.tracer_courant returns: rdt * min(face_limit / face_max, outflow_limit / outflow_max); inf when both
    maxima are 0"""
    best = math.inf
    if rec.face_max > 0.0:
        best = min(best, _div(face_limit, rec.face_max))
    if rec.outflow_max > 0.0:
        best = min(best, _div(outflow_limit, rec.outflow_max))
    return rdt * best if best != math.inf else math.inf
