"""Independent CPU evaluation of the flow step's stability check of DESIGN.md section 6.15.

TEST INFRASTRUCTURE.  The reference holds no such diagnostic, so its specification is frozen in DESIGN.md section 6.15 and
nothing in the reference can pin it.  Two evaluations are written here from that text, separately:
  * whole-array numpy expressions (`flow_courant`) over shifted views of the box;
  * a plain scalar loop (`flow_courant_scalar`), one cell at a time, line by line, that keeps the running extremes with their
    first (= lowest) index.
Both round every operation in double precision in the association order the parentheses give and choose with selects; numpy's
and math's sqrt and the division are correctly rounded.  Every member of the record is a maximum, a minimum, an integer or a
lowest index, so the two are required to agree with each other, and with the GPU, in every member exactly -- the doubles by
value (the sign of a zero is unspecified).

The box is 1-based inclusive with a one-cell ring inside the array; arrays are (ny, ld), [j, i] 0-based.
"""
import collections
import math

import numpy as np

from tracer_numpy import _div, _view

DBL_MAX = float(np.finfo(np.float64).max)
MEMBERS = ("gravity_max", "advective_max", "viscous_max", "depth_min", "gravity_index", "advective_index", "viscous_index",
           "depth_index", "gravity_over", "advective_over", "viscous_over", "shallow", "invalid", "wet")
Record = collections.namedtuple("Record", MEMBERS)
EMPTY = Record(0.0, 0.0, 0.0, math.inf, -1, -1, -1, -1, 0, 0, 0, 0, 0, 0)
LIMITS = (1.0, 1.0, 0.25, 0.0)          # gravity, advective, viscous, depth


def _valid(x):
    with np.errstate(all="ignore"):
        return (x >= 0.0) & (x <= DBL_MAX)


def cells(rdt, g, visc, box, tmask, dx_t, dy_t, un, vn, ht, sshn_t):
    """per-cell values of section 6.15 over the box, as a dict: wet, d, gw, adv, vis, bad (bad of wet cells only), and the
    operands a1..a4 of the two selects"""
    S = _view(box)
    T = tmask
    rdt, g, visc = np.float64(rdt), np.float64(g), np.float64(visc)
    wet = S(T) > 0
    with np.errstate(all="ignore"):
        d = S(ht) + S(sshn_t)
        ix, iy = 1.0 / S(dx_t), 1.0 / S(dy_t)
        k2 = ix * ix + iy * iy
        gw = (rdt * np.sqrt(g * d)) * np.sqrt(k2)
        a1 = np.where(S(T, 1, 0) != 0, np.abs(S(un)), 0.0)
        a2 = np.where(S(T, -1, 0) != 0, np.abs(S(un, -1, 0)), 0.0)
        a3 = np.where(S(T, 0, 1) != 0, np.abs(S(vn)), 0.0)
        a4 = np.where(S(T, 0, -1) != 0, np.abs(S(vn, 0, -1)), 0.0)
        um = np.where(a1 >= a2, a1, a2)
        vm = np.where(a3 >= a4, a3, a4)
        adv = (rdt * um) * ix + (rdt * vm) * iy
        vis = (rdt * visc) * k2
        bad = ~((d > 0.0) & (d <= DBL_MAX))
        for x in (a1, a2, a3, a4, gw, adv, vis):
            bad = bad | ~_valid(x)
    return dict(wet=wet, d=d, gw=gw, adv=adv, vis=vis, bad=wet & bad, a=(a1, a2, a3, a4))


def flow_courant(rdt, g, visc, box, tmask, dx_t, dy_t, un, vn, ht, sshn_t, gravity_limit=1.0, advective_limit=1.0,
                 viscous_limit=0.25, depth_limit=0.0):
    """DESIGN.md section 6.15 on whole arrays"""
    xs, xe, ys, ye = box
    if xe < xs or ye < ys:
        return EMPTY
    ny, ld = tmask.shape
    assert xs >= 2 and ys >= 2 and xe <= ld - 1 and ye <= ny - 1                      # the ring: no view wraps
    c = cells(rdt, g, visc, box, tmask, dx_t, dy_t, un, vn, ht, sshn_t)
    ok = c["wet"] & ~c["bad"]
    jj, ii = np.mgrid[ys - 1:ye, xs - 1:xe]
    index = jj.astype(np.int64) * ld + ii

    def extreme(x, pick, none):
        if not ok.any():
            return none, -1
        best = pick(x[ok])
        return float(best), int(index[ok & (x == best)].min())
    gm, gi = extreme(c["gw"], np.max, 0.0)
    am, ai = extreme(c["adv"], np.max, 0.0)
    vm, vi = extreme(c["vis"], np.max, 0.0)
    dm, di = extreme(c["d"], np.min, math.inf)

    def count(cond):
        with np.errstate(all="ignore"):
            return int((ok & cond).sum())
    return Record(gm, am, vm, dm, gi, ai, vi, di, count(c["gw"] >= gravity_limit), count(c["adv"] >= advective_limit),
                  count(c["vis"] >= viscous_limit), count(c["d"] <= depth_limit), int(c["bad"].sum()), int(c["wet"].sum()))


def _valid_scalar(x):
    return x >= 0.0 and x <= DBL_MAX


def _sqrt(x):
    """IEEE square root of a double: NaN for a negative number (math.sqrt raises) and for a NaN"""
    return math.sqrt(x) if x >= 0.0 else (x if x == 0.0 else math.nan)


def flow_courant_scalar(rdt, g, visc, box, tmask, dx_t, dy_t, un, vn, ht, sshn_t, gravity_limit=1.0, advective_limit=1.0,
                        viscous_limit=0.25, depth_limit=0.0):
    """the same rule, one cell at a time; i, j are 0-based here"""
    xs, xe, ys, ye = box
    rdt, g, visc = float(rdt), float(g), float(visc)
    ny, ld = tmask.shape
    best = {"g": None, "a": None, "v": None, "d": None}
    at = {"g": -1, "a": -1, "v": -1, "d": -1}
    over_g = over_a = over_v = shallow = invalid = wet = 0
    for j in range(ys - 1, ye):
        for i in range(xs - 1, xe):
            if tmask[j, i] <= 0:
                continue
            assert 1 <= i <= ld - 2 and 1 <= j <= ny - 2          # the ring
            wet += 1
            d = float(ht[j, i]) + float(sshn_t[j, i])
            ix, iy = _div(1.0, dx_t[j, i]), _div(1.0, dy_t[j, i])
            k2 = ix * ix + iy * iy
            gw = (rdt * _sqrt(g * d)) * _sqrt(k2)
            a1 = abs(float(un[j, i])) if tmask[j, i + 1] != 0 else 0.0
            a2 = abs(float(un[j, i - 1])) if tmask[j, i - 1] != 0 else 0.0
            a3 = abs(float(vn[j, i])) if tmask[j + 1, i] != 0 else 0.0
            a4 = abs(float(vn[j - 1, i])) if tmask[j - 1, i] != 0 else 0.0
            um = a1 if a1 >= a2 else a2
            vm = a3 if a3 >= a4 else a4
            adv = (rdt * um) * ix + (rdt * vm) * iy
            vis = (rdt * visc) * k2
            if not (d > 0.0 and d <= DBL_MAX) or not all(_valid_scalar(x) for x in (a1, a2, a3, a4, gw, adv, vis)):
                invalid += 1
                continue
            here = j * ld + i
            for key, x in (("g", gw), ("a", adv), ("v", vis), ("d", -d)):
                if best[key] is None or x > best[key]:            # cells come in index order: the first one stays
                    best[key], at[key] = x, here
            over_g += gw >= gravity_limit
            over_a += adv >= advective_limit
            over_v += vis >= viscous_limit
            shallow += d <= depth_limit
    if best["g"] is None:
        return EMPTY._replace(invalid=invalid, wet=wet)
    return Record(best["g"], best["a"], best["v"], -best["d"], at["g"], at["a"], at["v"], at["d"], int(over_g), int(over_a),
                  int(over_v), int(shallow), invalid, wet)


def same_record(a, b):
    """every member equal: the doubles by value (none is a NaN), the integers exactly"""
    a, b = Record(*a), Record(*b)
    return (not any(math.isnan(x) for x in a[:4]) and tuple(a[:4]) == tuple(b[:4])
            and tuple(int(x) for x in a[4:]) == tuple(int(x) for x in b[4:]))


def rdt_limit(rdt, rec, gravity_limit=1.0, advective_limit=1.0, viscous_limit=0.25):
    """the estimate psy.flow_courant returns: rdt * min(limit / maximum) over the maxima that are not 0; inf when all are"""
    best = math.inf
    for lim, top in ((gravity_limit, rec.gravity_max), (advective_limit, rec.advective_max), (viscous_limit, rec.viscous_max)):
        if top > 0.0:
            best = min(best, _div(lim, top))
    return rdt * best if best != math.inf else math.inf
