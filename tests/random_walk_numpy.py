"""Two independent CPU restatements of the random walk in a varying diffusivity, built on
dispersal_numpy's Philox and drifter_numpy's velocity rule: random_walk_scalar walks one particle at a time through the rule
as it is written, random_walk follows all particles at once with masks and never branches on a particle.  Arrays, boxes, the
seed, the ids and the in-place convention are dispersal_numpy's; kh_t is an (ny, ld) array like dx_t.

Both keep the same census, counted over the substeps of particles that are ACTIVE on a wet cell when the substep begins:
    coast_face   faces (of four) whose neighbour is land: the face takes the cell's own value
    open_read    faces whose neighbour is an open cell: its kh_t is read and used
    clamped      axes whose diffusivity half a drift ahead is not > 0 and is taken as 0
    rejected     kicks that end on land
    left, open, grounded   particles that end the substep with that status

naive=True is the scheme the rule replaces, for the well-mixed test alone: no drift, K = the own cell's value.
"""
import numpy as np

import dispersal_numpy as PN
import drifter_numpy as DN
from drifter_numpy import ACTIVE, LEFT, OPEN, GROUNDED

F = np.float64
CENSUS = ("coast_face", "open_read", "clamped", "rejected", "left", "open", "grounded")


def _axis(ah, d, frac, t_hi, t_lo, kc, k_hi, k_lo, r, naive, note):
    """the kick along one axis, in cells: d = the metric, frac = the particle's place in its cell, hi = east or north"""
    for t in (t_hi, t_lo):
        if t == 0:
            note("coast_face")
        elif t < 0:
            note("open_read")
    f_hi = F(0.5) * (kc + k_hi) if t_hi != 0 else kc
    f_lo = F(0.5) * (kc + k_lo) if t_lo != 0 else kc
    dk = f_hi - f_lo
    c = (ah * dk) / (d * d)
    k = f_lo + dk * (frac + F(0.5) * c)
    if naive:
        c, k = F(0.0), kc
    if not k > 0.0:
        note("clamped")
        k = F(0.0)
    return c + (np.sqrt((F(6.0) * k) * ah) * r) / d


# ---------------------------------------------------------------------------------------------- one particle at a time
def particle(h, nsub, kh_t, seed, tick, box, tm, dx_t, dy_t, un, vn, x, y, ident, census=None, naive=False):
    """(x, y, status) of one ACTIVE particle of identity `ident` (32 bits) after one call"""
    def note(key):
        if census is not None:
            census[key] = census.get(key, 0) + 1
    x, y = F(x), F(y)
    ah = np.abs(F(h))
    key = PN._key(seed)
    if not DN.inbox(box, x, y):
        return x, y, LEFT
    i, j = DN._cell(x, y)
    if tm[j - 1, i - 1] < 0:
        return x, y, OPEN
    if tm[j - 1, i - 1] == 0:
        return x, y, GROUNDED
    for s in range(nsub):
        tau = int(tick) + s
        w = PN.philox((int(ident), 0, tau & PN.MASK32, tau >> 32), key)
        i, j = DN._cell(x, y)
        J, I = j - 1, i - 1
        gx = _axis(ah, dx_t[J, I], x - F(i), tm[J, I + 1], tm[J, I - 1], kh_t[J, I], kh_t[J, I + 1], kh_t[J, I - 1],
                   PN.sym(w[0]), naive, note)
        gy = _axis(ah, dy_t[J, I], y - F(j), tm[J + 1, I], tm[J - 1, I], kh_t[J, I], kh_t[J + 1, I], kh_t[J - 1, I],
                   PN.sym(w[1]), naive, note)
        k1x, k1y = DN._vel(h, x, y, i, j, tm, dx_t, dy_t, un, vn)
        xm, ym = x + F(0.5) * k1x, y + F(0.5) * k1y
        k2x, k2y = k1x, k1y
        if DN.inbox(box, xm, ym):
            im, jm = DN._cell(xm, ym)
            if tm[jm - 1, im - 1] > 0:
                k2x, k2y = DN._vel(h, xm, ym, im, jm, tm, dx_t, dy_t, un, vn)
        xd, yd = x + k2x, y + k2y
        xa, ya = xd + gx, yd + gy
        if not DN.inbox(box, xa, ya):
            note("left")
            return xa, ya, LEFT
        i, j = DN._cell(xa, ya)
        if tm[j - 1, i - 1] != 0:
            x, y = xa, ya
            if tm[j - 1, i - 1] < 0:
                note("open")
                return x, y, OPEN
            continue
        note("rejected")
        if not DN.inbox(box, xd, yd):
            note("left")
            return xd, yd, LEFT
        i, j = DN._cell(xd, yd)
        if tm[j - 1, i - 1] == 0:
            note("grounded")
            return x, y, GROUNDED
        x, y = xd, yd
        if tm[j - 1, i - 1] < 0:
            note("open")
            return x, y, OPEN
    return x, y, ACTIVE


def random_walk_scalar(h, nsub, kh_t, seed, tick, box, tm, dx_t, dy_t, un, vn, px, py, status, ids=None, census=None,
                       naive=False):
    idv = PN._ids(ids, len(px))
    with np.errstate(all="ignore"):
        for p in range(len(px)):
            if status[p] != ACTIVE:
                continue
            px[p], py[p], status[p] = particle(h, nsub, kh_t, seed, tick, box, tm, dx_t, dy_t, un, vn, px[p], py[p],
                                               int(idv[p]), census, naive)


# ---------------------------------------------------------------------------------------------- all particles at once
def _axis_v(ah, d, frac, t_hi, t_lo, kc, k_hi, k_lo, r, naive, live, seen):
    f_hi, f_lo = np.where(t_hi != 0, 0.5 * (kc + k_hi), kc), np.where(t_lo != 0, 0.5 * (kc + k_lo), kc)
    dk = f_hi - f_lo
    c = (ah * dk) / (d * d)
    k = f_lo + dk * (frac + 0.5 * c)
    if naive:
        c, k = np.zeros(len(d)), kc
    pos = k > 0.0
    seen["coast_face"] += int((live & (t_hi == 0)).sum() + (live & (t_lo == 0)).sum())
    seen["open_read"] += int((live & (t_hi < 0)).sum() + (live & (t_lo < 0)).sum())
    seen["clamped"] += int((live & ~pos).sum())
    return c + (np.sqrt((6.0 * np.where(pos, k, 0.0)) * ah) * r) / d


def random_walk(h, nsub, kh_t, seed, tick, box, tm, dx_t, dy_t, un, vn, px, py, status, ids=None, census=None, naive=False):
    h = float(h)
    ah = abs(h)
    k0, k1 = PN._key(seed)
    idv = PN._ids(ids, len(px))
    seen = dict.fromkeys(CENSUS, 0)
    with np.errstate(all="ignore"):
        act = status == ACTIVE
        x, y, st = px.copy(), py.copy(), status.copy()
        home = np.full(len(x), box[2] - 1, dtype=np.int64), np.full(len(x), box[0] - 1, dtype=np.int64)
        ok = DN._inbox_v(box, x, y)
        J, I = DN._cells_v(ok, x, y, home[1], home[0])
        t = tm[J, I]
        st[act & ~ok] = LEFT
        st[act & ok & (t < 0)] = OPEN
        st[act & ok & (t == 0)] = GROUNDED
        live = act & ok & (t > 0)
        for s in range(nsub):
            tau = int(tick) + s
            w = PN.philox_v(idv, 0, tau & PN.MASK32, tau >> 32, k0, k1)
            gx = _axis_v(ah, dx_t[J, I], x - (I + 1).astype(np.float64), tm[J, I + 1], tm[J, I - 1], kh_t[J, I],
                         kh_t[J, I + 1], kh_t[J, I - 1], PN.sym_v(w[0]), naive, live, seen)
            gy = _axis_v(ah, dy_t[J, I], y - (J + 1).astype(np.float64), tm[J + 1, I], tm[J - 1, I], kh_t[J, I],
                         kh_t[J + 1, I], kh_t[J - 1, I], PN.sym_v(w[1]), naive, live, seen)
            k1x, k1y = DN._vel_v(h, x, y, J, I, tm, dx_t, dy_t, un, vn)
            xm, ym = x + 0.5 * k1x, y + 0.5 * k1y
            in_m = DN._inbox_v(box, xm, ym)
            Jm, Im = DN._cells_v(in_m, xm, ym, I, J)
            kmx, kmy = DN._vel_v(h, np.where(in_m, xm, x), np.where(in_m, ym, y), Jm, Im, tm, dx_t, dy_t, un, vn)
            mid = in_m & (tm[Jm, Im] > 0)
            xd, yd = x + np.where(mid, kmx, k1x), y + np.where(mid, kmy, k1y)
            xa, ya = xd + gx, yd + gy
            in_a, in_d = DN._inbox_v(box, xa, ya), DN._inbox_v(box, xd, yd)
            Ja, Ia = DN._cells_v(in_a, xa, ya, I, J)
            Jd, Id = DN._cells_v(in_d, xd, yd, I, J)
            ta, td = tm[Ja, Ia], tm[Jd, Id]
            left_a, take_a, rej = live & ~in_a, live & in_a & (ta != 0), live & in_a & (ta == 0)
            left_d, ground, take_d = rej & ~in_d, rej & in_d & (td == 0), rej & in_d & (td != 0)
            x = np.where(left_a | take_a, xa, np.where(left_d | take_d, xd, x))
            y = np.where(left_a | take_a, ya, np.where(left_d | take_d, yd, y))
            J, I = np.where(take_a, Ja, np.where(take_d, Jd, J)), np.where(take_a, Ia, np.where(take_d, Id, I))
            opened = (take_a & (ta < 0)) | (take_d & (td < 0))
            st[left_a | left_d] = LEFT
            st[ground] = GROUNDED
            st[opened] = OPEN
            live = (take_a & (ta > 0)) | (take_d & (td > 0))
            seen["rejected"] += int(rej.sum())
            seen["left"] += int((left_a | left_d).sum())
            seen["open"] += int(opened.sum())
            seen["grounded"] += int(ground.sum())
        px[act], py[act], status[act] = x[act], y[act], st[act]
    if census is not None:
        for k, v in seen.items():
            census[k] = census.get(k, 0) + v
