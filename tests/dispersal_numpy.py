"""Two independent CPU restatements of the dispersal rule, built on drifter_numpy's velocity rule:
dispersal_step_scalar walks one particle at a time through the rule as it is written, with Philox4x32-10 in Python integers;
dispersal_step follows all particles at once with masks, Philox in uint64 arrays, and never branches on a particle.  Arrays,
boxes and the in-place convention are drifter_numpy's.  seed: any Python integer, taken modulo 2^64; ids: None (the slot
number) or an int32 array, taken as 32 bits.
"""
import numpy as np

import drifter_numpy as DN
from drifter_numpy import ACTIVE, LEFT, OPEN, GROUNDED

F = np.float64
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32, MASK64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


# ---------------------------------------------------------------------------------------------- the generator
def philox(counter, key):
    """Philox4x32-10 in Python integers: (c0, c1, c2, c3), (k0, k1) -> four 32-bit words"""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def philox_v(c0, c1, c2, c3, k0, k1):
    """the same on arrays: every argument a uint64 array (or scalar) of values below 2^32; four uint64 arrays"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    m32, s32 = np.uint64(MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2              # < 2^64: no wrap
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + np.uint64(W0)) & m32, (k1 + np.uint64(W1)) & m32
    return c0, c1, c2, c3


def sym(w):
    """a 32-bit word -> the centre of its bin of (-1, 1), exactly"""
    return (F(w) + F(0.5)) * F(2.0 ** -31) - F(1.0)


def sym_v(w):
    return (w.astype(np.float64) + 0.5) * 2.0 ** -31 - 1.0


def amplitude(kh, h):
    return np.sqrt((F(6.0) * F(kh)) * np.abs(F(h)))


def _key(seed):
    seed = int(seed) & MASK64
    return seed & MASK32, seed >> 32


def _ids(ids, n):
    if ids is None:
        return (np.arange(n, dtype=np.int64) & MASK32).astype(np.uint64)
    return np.ascontiguousarray(ids, dtype=np.int32).view(np.uint32).astype(np.uint64)


# ---------------------------------------------------------------------------------------------- one particle at a time
def particle(h, nsub, kh, seed, tick, box, tm, dx_t, dy_t, un, vn, x, y, ident, census=None):
    """(x, y, status) of one ACTIVE particle of identity `ident` (32 bits) after one call; census counts the branches"""
    def note(key):
        if census is not None:
            census[key] = census.get(key, 0) + 1
    x, y = F(x), F(y)
    amp = amplitude(kh, h)
    key = _key(seed)
    if not DN.inbox(box, x, y):
        return x, y, LEFT
    i, j = DN._cell(x, y)
    if tm[j - 1, i - 1] < 0:
        return x, y, OPEN
    if tm[j - 1, i - 1] == 0:
        return x, y, GROUNDED
    for s in range(nsub):
        tau = int(tick) + s
        w = philox((int(ident), 0, tau & MASK32, tau >> 32), key)
        i, j = DN._cell(x, y)
        gx, gy = (amp * sym(w[0])) / dx_t[j - 1, i - 1], (amp * sym(w[1])) / dy_t[j - 1, i - 1]
        k1x, k1y = DN._vel(h, x, y, i, j, tm, dx_t, dy_t, un, vn)
        xm, ym = x + F(0.5) * k1x, y + F(0.5) * k1y
        k2x, k2y = k1x, k1y
        if DN.inbox(box, xm, ym):
            im, jm = DN._cell(xm, ym)
            if tm[jm - 1, im - 1] > 0:
                k2x, k2y = DN._vel(h, xm, ym, im, jm, tm, dx_t, dy_t, un, vn)
        xd, yd = x + k2x, y + k2y
        xa, ya = xd + gx, yd + gy
        d_wet = False
        if DN.inbox(box, xd, yd):
            i, j = DN._cell(xd, yd)
            d_wet = tm[j - 1, i - 1] > 0
        if not DN.inbox(box, xa, ya):
            note("left_by_kick" if DN.inbox(box, xd, yd) else "left")
            return xa, ya, LEFT
        i, j = DN._cell(xa, ya)
        if tm[j - 1, i - 1] != 0:
            x, y = xa, ya
            if tm[j - 1, i - 1] < 0:
                note("open_by_kick" if d_wet else "open")
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


def dispersal_step_scalar(h, nsub, kh, seed, tick, box, tm, dx_t, dy_t, un, vn, px, py, status, ids=None, census=None):
    idv = _ids(ids, len(px))
    with np.errstate(all="ignore"):
        for p in range(len(px)):
            if status[p] != ACTIVE:
                continue
            px[p], py[p], status[p] = particle(h, nsub, kh, seed, tick, box, tm, dx_t, dy_t, un, vn, px[p], py[p],
                                               int(idv[p]), census)


# ---------------------------------------------------------------------------------------------- all particles at once
def dispersal_step(h, nsub, kh, seed, tick, box, tm, dx_t, dy_t, un, vn, px, py, status, ids=None, census=None):
    """census: a dict that receives the numbers of kicks rejected on land, of particles LEFT and OPEN by the kick alone (the
    unkicked destination in the box, resp. on a wet cell of it) and of particles GROUNDED"""
    h = float(h)
    amp = float(amplitude(kh, h))
    k0, k1 = _key(seed)
    idv = _ids(ids, len(px))
    seen = dict(rejected=0, left_by_kick=0, open_by_kick=0, grounded=0)
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
            w = philox_v(idv, 0, tau & MASK32, tau >> 32, k0, k1)
            gx, gy = (amp * sym_v(w[0])) / dx_t[J, I], (amp * sym_v(w[1])) / dy_t[J, I]
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
            st[left_a | left_d] = LEFT
            st[ground] = GROUNDED
            st[(take_a & (ta < 0)) | (take_d & (td < 0))] = OPEN
            live = (take_a & (ta > 0)) | (take_d & (td > 0))
            seen["rejected"] += int(rej.sum())
            seen["left_by_kick"] += int((left_a & in_d).sum())
            seen["open_by_kick"] += int((take_a & (ta < 0) & in_d & (td > 0)).sum())
            seen["grounded"] += int(ground.sum())
        px[act], py[act], status[act] = x[act], y[act], st[act]
    if census is not None:
        for k, v in seen.items():
            census[k] = census.get(k, 0) + v
