"""Independent CPU evaluation of the model's output fields of DESIGN.md section 6.16.

TEST INFRASTRUCTURE.  The reference's model_write holds the T-point velocities only and writes text; the six fields, the land
switches and the two store modes are frozen in DESIGN.md section 6.16 and nothing in the reference can pin them.  Two
evaluations are written here from that text, separately:
  * whole-array numpy expressions (`flow_output`) over shifted views of the box;
  * a plain scalar loop (`flow_output_scalar`), one cell at a time, line by line.
Both round every operation in double precision in the association order the parentheses give and choose with selects; numpy's
and math's sqrt and the division are correctly rounded.  The two are required to agree with each other, and with the GPU, bit
for bit in every cell of every array, any NaN equal to any NaN (`same`: the sign and payload of a generated NaN are not
specified and differ between x86 and the GPU).

The box is 1-based inclusive with a one-cell ring inside the array; arrays are (ny, ld), [j, i] 0-based.  `out` is a list of
six arrays or None in the order SSH, UT, VT, SPEED, KE, VORT; an input no wanted output reads may be None and is not read.
"""
import math

import numpy as np

from momentum_numpy import same  # noqa: F401  (bit for bit, any NaN equal to any NaN)
from tracer_numpy import _div, _view

SSH, UT, VT, SPEED, KE, VORT, COUNT = range(7)
NAMES = ("ssh", "ut", "vt", "speed", "ke", "vort")
SET, ADD = 0, 1


def needs(out):
    """which of (dx_v, dy_u, un, vn, ht, sshn_t) the wanted outputs read"""
    vort, ke, ssh = out[VORT] is not None, out[KE] is not None, out[SSH] is not None
    return (vort, vort, True, True, ke, ssh or ke)


def corner_of(tmask, box):
    """corner over the box: the cells east, north and north-east are not land"""
    S = _view(box)
    return (S(tmask, 1, 0) != 0) & (S(tmask, 0, 1) != 0) & (S(tmask, 1, 1) != 0)


def written(tmask, box, k):
    """the cells output k is stored in, over the whole array"""
    xs, xe, ys, ye = box
    w = np.zeros(tmask.shape, dtype=bool)
    if xe < xs or ye < ys:
        return w
    S = _view(box)
    w[ys - 1:ye, xs - 1:xe] = (S(tmask) > 0) & (corner_of(tmask, box) if k == VORT else True)
    return w


def flow_output(mode, weight, box, tmask, dx_v, dy_u, un, vn, ht, sshn_t, out):
    """DESIGN.md section 6.16 on whole arrays, in place"""
    xs, xe, ys, ye = box
    if xe < xs or ye < ys:
        return
    ny, ld = tmask.shape
    assert xs >= 2 and ys >= 2 and xe <= ld - 1 and ye <= ny - 1                      # the ring: no view wraps
    S = _view(box)
    T = tmask
    wet = S(T) > 0
    value = [None] * COUNT
    with np.errstate(all="ignore"):
        e = np.where(S(T, 1, 0) != 0, S(un), 0.0)
        w = np.where(S(T, -1, 0) != 0, S(un, -1, 0), 0.0)
        n = np.where(S(T, 0, 1) != 0, S(vn), 0.0)
        s = np.where(S(T, 0, -1) != 0, S(vn, 0, -1), 0.0)
        ut, vt = 0.5 * (w + e), 0.5 * (s + n)
        q = ut * ut + vt * vt
        value[UT], value[VT], value[SPEED] = ut, vt, np.sqrt(q)
        if out[SSH] is not None:
            value[SSH] = S(sshn_t)
        if out[KE] is not None:
            value[KE] = (0.5 * (S(ht) + S(sshn_t))) * q
        if out[VORT] is not None:
            dvdx = (S(vn, 1, 0) - S(vn)) / (0.5 * (S(dx_v) + S(dx_v, 1, 0)))
            dudy = (S(un, 0, 1) - S(un)) / (0.5 * (S(dy_u) + S(dy_u, 0, 1)))
            value[VORT] = dvdx - dudy
        for k in range(COUNT):
            if out[k] is None:
                continue
            store = wet & corner_of(T, box) if k == VORT else wet
            new = value[k] if mode == SET else S(out[k]) + np.float64(weight) * value[k]
            S(out[k])[store] = new[store]


def _sqrt(x):
    """IEEE square root of a double: NaN for a negative number (math.sqrt raises) and for a NaN"""
    return math.sqrt(x) if x >= 0.0 else (x if x == 0.0 else math.nan)


def _mul(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) * np.float64(b))


def _add(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) + np.float64(b))


def flow_output_scalar(mode, weight, box, tmask, dx_v, dy_u, un, vn, ht, sshn_t, out):
    """the same rule, one cell at a time; i, j are 0-based here"""
    xs, xe, ys, ye = box
    ny, ld = tmask.shape
    weight = float(weight)
    for j in range(ys - 1, ye):
        for i in range(xs - 1, xe):
            if tmask[j, i] <= 0:
                continue
            assert 1 <= i <= ld - 2 and 1 <= j <= ny - 2          # the ring
            e = float(un[j, i]) if tmask[j, i + 1] != 0 else 0.0
            w = float(un[j, i - 1]) if tmask[j, i - 1] != 0 else 0.0
            n = float(vn[j, i]) if tmask[j + 1, i] != 0 else 0.0
            s = float(vn[j - 1, i]) if tmask[j - 1, i] != 0 else 0.0
            ut, vt = _mul(0.5, _add(w, e)), _mul(0.5, _add(s, n))
            q = _add(_mul(ut, ut), _mul(vt, vt))
            value = [None, ut, vt, _sqrt(q), None, None]
            if out[SSH] is not None:
                value[SSH] = float(sshn_t[j, i])
            if out[KE] is not None:
                value[KE] = _mul(_mul(0.5, _add(ht[j, i], sshn_t[j, i])), q)
            if out[VORT] is not None and tmask[j, i + 1] != 0 and tmask[j + 1, i] != 0 and tmask[j + 1, i + 1] != 0:
                dvdx = _div(_add(vn[j, i + 1], -float(vn[j, i])), _mul(0.5, _add(dx_v[j, i], dx_v[j, i + 1])))
                dudy = _div(_add(un[j + 1, i], -float(un[j, i])), _mul(0.5, _add(dy_u[j, i], dy_u[j + 1, i])))
                value[VORT] = _add(dvdx, -dudy)
            for k in range(COUNT):
                if out[k] is None or value[k] is None:
                    continue
                out[k][j, i] = value[k] if mode == SET else _add(out[k][j, i], _mul(weight, value[k]))
