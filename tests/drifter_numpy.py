"""Two independent CPU restatements of the drifter rule: drifter_step_scalar walks one particle at a
time through the rule as it is written, drifter_step follows all particles at once with masks and never branches on a
particle.  Arrays are (ny, ld) numpy arrays, cell (i, j) of the rule is [j - 1, i - 1]; box = (xstart, xstop, ystart, ystop),
1-based inclusive.  Every operation is one rounded f64 operation in the rule's order.  Both work in place on px, py, status.
"""
import math

import numpy as np

ACTIVE, LEFT, OPEN, GROUNDED = range(4)
MAX_SUB, MAX_FIELDS = 1024, 8
F = np.float64


def same(a, b):
    """equal bit for bit, any NaN equal to any NaN (the sign and payload of a NaN an operation makes are the machine's)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != np.float64:
        return a.shape == b.shape and bool((a == b).all())
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


# ---------------------------------------------------------------------------------------------- one particle at a time
def inbox(box, x, y):
    xs, xe, ys, ye = box
    return bool(x >= F(xs) and x < F(xe) + F(1.0) and y >= F(ys) and y < F(ye) + F(1.0))


def _vel(h, x, y, i, j, tm, dx_t, dy_t, un, vn):
    J, I = j - 1, i - 1
    ue = un[J, I] if tm[J, I + 1] != 0 else F(0.0)
    uw = un[J, I - 1] if tm[J, I - 1] != 0 else F(0.0)
    vn_ = vn[J, I] if tm[J + 1, I] != 0 else F(0.0)
    vs = vn[J - 1, I] if tm[J - 1, I] != 0 else F(0.0)
    a, b = x - F(i), y - F(j)
    up = uw + (ue - uw) * a
    vp = vs + (vn_ - vs) * b
    return (F(h) * up) / dx_t[J, I], (F(h) * vp) / dy_t[J, I]


def _cell(x, y):
    return int(math.floor(x)), int(math.floor(y))


def particle(h, nsub, box, tm, dx_t, dy_t, un, vn, x, y, census=None):
    """(x, y, status) of one ACTIVE particle after one call; census: a dict that counts the branches taken"""
    def note(key):
        if census is not None:
            census[key] = census.get(key, 0) + 1
    x, y = F(x), F(y)
    if not inbox(box, x, y):
        note("entry_left")
        return x, y, LEFT
    i, j = _cell(x, y)
    if tm[j - 1, i - 1] < 0:
        note("entry_open")
        return x, y, OPEN
    if tm[j - 1, i - 1] == 0:
        note("entry_land")
        return x, y, GROUNDED
    note("entry_wet")
    for _ in range(nsub):
        i, j = _cell(x, y)
        k1x, k1y = _vel(h, x, y, i, j, tm, dx_t, dy_t, un, vn)
        xm, ym = x + F(0.5) * k1x, y + F(0.5) * k1y
        k2x, k2y = k1x, k1y
        if not inbox(box, xm, ym):
            note("mid_outside")
        else:
            im, jm = _cell(xm, ym)
            if tm[jm - 1, im - 1] > 0:
                note("mid_used")
                k2x, k2y = _vel(h, xm, ym, im, jm, tm, dx_t, dy_t, un, vn)
            else:
                note("mid_open" if tm[jm - 1, im - 1] < 0 else "mid_land")
        xn, yn = x + k2x, y + k2y
        if not inbox(box, xn, yn):
            note("move_left")
            return xn, yn, LEFT
        i, j = _cell(xn, yn)
        if tm[j - 1, i - 1] == 0:
            note("move_grounded")
            return x, y, GROUNDED
        x, y = xn, yn
        if tm[j - 1, i - 1] < 0:
            note("move_open")
            return x, y, OPEN
    return x, y, ACTIVE


def drifter_step_scalar(h, nsub, box, tm, dx_t, dy_t, un, vn, px, py, status, census=None):
    with np.errstate(all="ignore"):
        for p in range(len(px)):
            if status[p] != ACTIVE:
                continue
            px[p], py[p], status[p] = particle(h, nsub, box, tm, dx_t, dy_t, un, vn, px[p], py[p], census)


# ---------------------------------------------------------------------------------------------- all particles at once
def _inbox_v(box, x, y):
    xs, xe, ys, ye = box
    with np.errstate(invalid="ignore"):
        return (x >= xs) & (x < xe + 1.0) & (y >= ys) & (y < ye + 1.0)


def _cells_v(ok, x, y, i0, j0):
    """0-based (row, column) of cell(x, y) where ok, of the fall-back cell elsewhere (nothing that is not in the box is cast)"""
    return (np.where(ok, np.floor(np.where(ok, y, 1.0)), j0 + 1).astype(np.int64) - 1,
            np.where(ok, np.floor(np.where(ok, x, 1.0)), i0 + 1).astype(np.int64) - 1)


def _vel_v(h, x, y, J, I, tm, dx_t, dy_t, un, vn):
    zero = np.zeros(len(x))
    ue = np.where(tm[J, I + 1] != 0, un[J, I], zero)
    uw = np.where(tm[J, I - 1] != 0, un[J, I - 1], zero)
    vn_ = np.where(tm[J + 1, I] != 0, vn[J, I], zero)
    vs = np.where(tm[J - 1, I] != 0, vn[J - 1, I], zero)
    a, b = x - (I + 1).astype(np.float64), y - (J + 1).astype(np.float64)
    up = uw + (ue - uw) * a
    vp = vs + (vn_ - vs) * b
    return (h * up) / dx_t[J, I], (h * vp) / dy_t[J, I]


def drifter_step(h, nsub, box, tm, dx_t, dy_t, un, vn, px, py, status):
    h = float(h)
    with np.errstate(all="ignore"):
        act = status == ACTIVE
        x, y, st = px.copy(), py.copy(), status.copy()
        home = np.full(len(x), box[2] - 1, dtype=np.int64), np.full(len(x), box[0] - 1, dtype=np.int64)
        ok = _inbox_v(box, x, y)
        J, I = _cells_v(ok, x, y, home[1], home[0])
        t = tm[J, I]
        st[act & ~ok] = LEFT
        st[act & ok & (t < 0)] = OPEN
        st[act & ok & (t == 0)] = GROUNDED
        live = act & ok & (t > 0)
        for _ in range(nsub):
            k1x, k1y = _vel_v(h, x, y, J, I, tm, dx_t, dy_t, un, vn)
            xm, ym = x + 0.5 * k1x, y + 0.5 * k1y
            in_m = _inbox_v(box, xm, ym)
            Jm, Im = _cells_v(in_m, xm, ym, I, J)
            kmx, kmy = _vel_v(h, np.where(in_m, xm, x), np.where(in_m, ym, y), Jm, Im, tm, dx_t, dy_t, un, vn)
            mid = in_m & (tm[Jm, Im] > 0)
            xn, yn = x + np.where(mid, kmx, k1x), y + np.where(mid, kmy, k1y)
            in_n = _inbox_v(box, xn, yn)
            Jn, In = _cells_v(in_n, xn, yn, I, J)
            tn = tm[Jn, In]
            left, ground, move = live & ~in_n, live & in_n & (tn == 0), live & in_n & (tn != 0)
            x, y = np.where(left | move, xn, x), np.where(left | move, yn, y)
            J, I = np.where(move, Jn, J), np.where(move, In, I)
            st[left] = LEFT
            st[ground] = GROUNDED
            st[move & (tn < 0)] = OPEN
            live = move & (tn > 0)
        px[act], py[act], status[act] = x[act], y[act], st[act]


# ---------------------------------------------------------------------------------------------- sampling
def drifter_sample(box, px, py, status, fields, out):
    """out[k][p] = fields[k](cell(px, py)) for every ACTIVE particle in the box; everything else keeps its content"""
    ok = (status == ACTIVE) & _inbox_v(box, px, py)
    zero = np.zeros(len(px), dtype=np.int64)
    J, I = _cells_v(ok, px, py, zero, zero)
    for f, o in zip(fields, out):
        o[ok] = f[J[ok], I[ok]]
