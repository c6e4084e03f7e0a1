"""Test helpers of the NEMOLite2D-class kernels (DESIGN.md sections 6.5-6.7): the inputs of the GPU tests, and a seeded
generator of boxes whose edges fall where the two wave tiles branch.

The tiles (momentum_tile in dlesm_momentum.hip, nemolite_step_tile in dlesm_nemolite_step.hip) sweep chunks of 2 columns,
anchored at c_first = (x0 // 2) & ~7 (0-based x0 of the box swept, a 128-byte line); a momentum wave covers 64 chunks, a
step wave 63 (its lane 63 only loads, the next wave's lane 0).  `geometry` names the classes of edge placement a box takes
for a tile width; `cases` lists fixed boxes that reach every class for both widths, then random ones.

A case is (ld, ny, tbox, ubox, vbox, shift): arrays of (ny, ld), 1-based inclusive boxes inside a one-cell ring
(2 <= xstart, xstop <= ld - 1, the same in y) or empty (xstop < xstart), shift = 1: bases 8 bytes off a 16-byte boundary.
Nothing here needs a GPU; the device helpers import torch's module from their caller.
"""
import ctypes as C
import math
from collections import namedtuple

import numpy as np

import momentum_numpy as M

PRM = (20.0, 0.00015, 50.0, 9.80665)          # rdt, cbfr, visc, g
METRICS = ("dx_t", "dy_t", "dx_u", "dy_u", "dx_v", "dy_v", "area_t", "area_u", "area_v")
INS = ("un", "vn", "ht", "hu", "hv", "sshn_t", "sshn_u", "sshn_v")
OUTS = ("ssha", "ssha_u", "ssha_v", "ua", "va")
MOM = ("un", "vn", "ht", "sshn_t", "hu", "sshn_u", "hv", "sshn_v", "ssha_u", "ssha_v")

Case = namedtuple("Case", "ld ny tbox ubox vbox shift")


# ---- inputs ---------------------------------------------------------------------------------------------------------
def _vel(rng, shape):
    v = rng.normal(0.0, 0.3, shape)
    pick = rng.random(shape)
    v[pick < 0.15] = 0.0
    v[(pick >= 0.15) & (pick < 0.3)] = -0.0
    return v


def _host_inputs(rng, shape):
    """un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v"""
    H = {"un": _vel(rng, shape), "vn": _vel(rng, shape)}
    for k in ("ht", "hu", "hv"):
        H[k] = 10.0 + rng.random(shape)
    for k in ("sshn_t", "sshn_u", "sshn_v"):
        H[k] = 0.1 * rng.normal(size=shape)
    return H


def _host_outputs(rng, shape):
    """ssha: distinct values everywhere (the ring's are read by next_ssh*, the box's overwritten); the others sentinels"""
    H = {"ssha": 1000.0 + rng.random(shape)}
    for k in OUTS[1:]:
        H[k] = np.full(shape, -7.0)
    return H


def mask(rng, ny, ld):
    """a random -1/0/1 mask the open-boundary plan accepts on every box"""
    import open_bc_numpy as B
    return B.repair(rng.choice(np.array([-1, 0, 1, 1, 1], dtype=np.int32), size=(ny, ld)))


def host_grid(rng, tm):
    """non-uniform metrics (zero T spacings on land: dry cells divide by zero) and a varying Coriolis parameter, area_t
    beside them, as a dict of host arrays"""
    ny, ld = tm.shape
    G = {"tmask": np.ascontiguousarray(tm, dtype=np.int32)}
    land = tm <= 0
    for name in METRICS:
        a = 900.0 + 200.0 * rng.random((ny, ld))
        if name.startswith("area"):
            a *= 1000.0
        elif name.endswith("_t"):
            a[land] = 0.0
        G[name] = a
    G["fcor_u"] = M.coriolis(40.0 + 20.0 * rng.random((ny, ld)), 7.292116e-5, math.pi / 180.0)
    G["fcor_v"] = M.coriolis(40.0 + 20.0 * rng.random((ny, ld)), 7.292116e-5, math.pi / 180.0)
    return G


def grid_on_device(torch, G):
    """(host namespace, device arrays, dlesm_momentum_grid) of a host_grid dict"""
    dev = {k: torch.from_numpy(v).cuda() for k, v in G.items()}
    from dl_esm_inf_amd import _cabi
    mg = _cabi.MomentumGrid(**{k: dev[k].data_ptr() for k in M.GRID_ARRAYS})
    return M.SimpleNamespace(**G), dev, mg


def _raw_grid(torch, rng, tm):
    """a dlesm_momentum_grid of host_grid's arrays; host copies in G"""
    return grid_on_device(torch, host_grid(rng, tm))


def _dev(torch, host, shift):
    """device copies; shift: bases 8 bytes off a 16-byte boundary"""
    out = {}
    for k, a in host.items():
        t = torch.from_numpy(a.copy()).cuda()
        if shift:
            t = torch.cat([torch.zeros(1, dtype=torch.float64, device="cuda"), t.flatten()])[1:].view(a.shape)
        out[k] = t
    return out


def _plan(D, tm, tbox, ubox, vbox):
    ny, ld = tm.shape
    tm = np.ascontiguousarray(tm, dtype=np.int32)
    h = C.c_void_p()
    D._cabi.check(D._cabi.lib().dlesm_obc_create(tm.ctypes.data, ld, ny, C.byref(D._cabi.Region(0, 0, *tbox)),
                                                 C.byref(D._cabi.Region(0, 0, *ubox)), C.byref(D._cabi.Region(0, 0, *vbox)),
                                                 C.byref(h)))
    return h


# ---- IEEE special values ------------------------------------------------------------------------------------------
TINY = 2.2250738585072014e-308                # the smallest normal double
SPECIAL = np.array([5e-324, -5e-324, 2.5e-310, -1.0e-309, 0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1e300, -1e300,
                    1e154, -1e154])


def special_inputs(seed, ld, ny):
    """(tmask, host grid dict, inputs, outputs) seeded with subnormals, signed zeros, infinities, NaN of both signs, values
    near the overflow threshold, and cells where a denominator is exactly zero:
      * hu + ssha_u = 0 and hv + ssha_v = 0 (momentum's inputs ssha_u / ssha_v);
      * in a calm patch (velocities and sshn_t zero, hu = hv = 0) the step's own ssha, ssha_u, ssha_v are zero, so its
        denominators hu + ssha_u and hv + ssha_v are zero there;
      * dx_t = dy_t = 0 on wet cells beside wet cells;
    and a patch of subnormal velocities whose updates stay subnormal.  Inputs hold MOM's ten arrays."""
    rng = np.random.default_rng(seed)
    tm = mask(rng, ny, ld)
    G = host_grid(rng, tm)
    shape = (ny, ld)
    H = _host_inputs(rng, shape)
    H["ssha_u"] = 0.1 * rng.normal(size=shape)
    H["ssha_v"] = 0.1 * rng.normal(size=shape)
    O_ = _host_outputs(rng, shape)
    for k, dens in (("un", 0.03), ("vn", 0.03), ("sshn_t", 0.01), ("sshn_u", 0.01), ("sshn_v", 0.01), ("hu", 0.005),
                    ("hv", 0.005), ("ht", 0.005), ("ssha_u", 0.005), ("ssha_v", 0.005)):
        pick = rng.random(shape) < dens
        H[k][pick] = rng.choice(SPECIAL, size=int(pick.sum()))
    for name in ("dx_u", "dy_u", "dx_v", "dy_v", "area_u", "area_v", "fcor_u", "fcor_v"):
        pick = rng.random(shape) < 0.002
        G[name][pick] = rng.choice(SPECIAL, size=int(pick.sum()))
    wet = tm > 0
    # momentum's zero denominators
    for h, s in (("hu", "ssha_u"), ("hv", "ssha_v")):
        pick = (rng.random(shape) < 0.03) & wet
        H[s][pick] = -H[h][pick]
    # zero T spacings on wet cells
    for name in ("dx_t", "dy_t"):
        pick = (rng.random(shape) < 0.02) & wet
        G[name][pick] = 0.0
    # the step's zero denominators: a calm patch
    j0, i0 = ny // 3, ld // 3
    sl = (slice(j0, j0 + 3), slice(i0, i0 + 6))
    for k in ("un", "vn", "sshn_t", "sshn_u", "sshn_v", "hu", "hv"):
        H[k][sl] = 0.0
    tm[sl] = 1
    # subnormal velocities in a quiet patch of uniform depth and surface
    j1, i1 = 2 * ny // 3, 2 * ld // 3
    sl = (slice(j1 - 1, j1 + 2), slice(max(i1 - 4, 1), i1 + 4))
    for k in ("un", "vn"):
        H[k][sl] = 2.5e-310 * (1.0 + rng.random(H[k][sl].shape))
    for k in ("sshn_t", "sshn_u", "sshn_v"):
        H[k][sl] = 0.0
    for k in ("ht", "hu", "hv"):
        H[k][sl] = 10.0
    tm[sl] = 1
    G["tmask"] = np.ascontiguousarray(tm, dtype=np.int32)
    return tm, G, H, O_


def is_subnormal(a):
    a = np.abs(np.asarray(a))
    return (a > 0.0) & (a < TINY)


# ---- boxes --------------------------------------------------------------------------------------------------------
WIDTHS = (63, 64)        # chunks per wave: the step tile, the momentum tile
EMPTY = (5, 4, 2, 2)


def empty(box):
    return box[1] < box[0] or box[3] < box[2]


def _b(x0, x1, y0, y1):
    """1-based box of 0-based inclusive columns / rows"""
    return (x0 + 1, x1 + 1, y0 + 1, y1 + 1)


def bounding(ubox, vbox):
    """the box momentum_tile sweeps: the bounding box of the non-empty ones (None if both are empty)"""
    boxes = [b for b in (ubox, vbox) if not empty(b)]
    if not boxes:
        return None
    return (min(b[0] for b in boxes), max(b[1] for b in boxes), min(b[2] for b in boxes), max(b[3] for b in boxes))


def geometry(box, width, anchor_box=None):
    """the edge-placement classes of a non-empty 1-based box for a tile of `width` chunks per wave, the tile anchored on
    anchor_box (the box swept; default the box itself):
      ('parity', x0 % 2, x1 % 2), ('last_lane', lane of the last chunk), ('first_offset', first chunk - anchor) when < 8,
      ('first_wave', k) when the first chunk is lane 0 of wave k >= 1, ('spans_wave', k) when lane 0 of wave k is inside,
      ('cols', 1 | 2) for a box of one or two columns ('one_col_odd' when the one column is the second of its chunk),
      ('rows', 1 | 2), ('ys2',), ('ye_last', ) -- ye_last needs ny, see `classes`"""
    ab = anchor_box or box
    x0, x1 = box[0] - 1, box[1] - 1
    cf = ((ab[0] - 1) // 2) & ~7
    out = {("parity", x0 % 2, x1 % 2), ("last_lane", (x1 // 2 - cf) % width)}
    d0 = x0 // 2 - cf
    if d0 < 8:
        out.add(("first_offset", d0))
    if d0 > 0 and d0 % width == 0:
        out.add(("first_wave", d0 // width))
    for k in range(1, (x1 // 2 - cf) // width + 1):
        if d0 <= k * width:
            out.add(("spans_wave", k))
    if x1 == x0:
        out.add(("cols", 1))
        if x0 % 2:
            out.add(("one_col_odd",))
    elif x1 == x0 + 1:
        out.add(("cols", 2))
    if box[3] == box[2]:
        out.add(("rows", 1))
    elif box[3] == box[2] + 1:
        out.add(("rows", 2))
    return out


def classes(case, width):
    """every class the case's boxes take for a tile width: the equal-box classes when tbox = ubox = vbox (the step tile's
    geometry), each of U and V against their bounding box otherwise (momentum_tile's), plus the case-level classes"""
    out = set()
    ld, ny, tb, ub, vb, shift = case
    for name, b in (("t", tb), ("u", ub), ("v", vb)):
        if not empty(b):
            anchor = None if name == "t" or tb == ub == vb else bounding(ub, vb)
            out |= geometry(b, width, anchor)
            if b[2] == 2:
                out.add(("ys2",))
            if b[3] == ny - 1:
                out.add(("ye_last",))
            if b == (2, ld - 1, 2, ny - 1):
                out.add(("ring", "small" if ld <= 130 else "large" if ld >= 1000 else "mid"))
    if empty(ub) and not empty(vb):
        out.add(("empty", "u"))
    if empty(vb) and not empty(ub):
        out.add(("empty", "v"))
    if empty(tb) and empty(ub) and empty(vb):
        out.add(("empty", "all"))
    if not empty(ub) and not empty(vb) and ub != vb:
        if all(ub[k] != vb[k] for k in range(4)):
            out.add(("uv_differ_every_edge",))
        if not (ub[1] < vb[0] or vb[1] < ub[0] or ub[3] < vb[2] or vb[3] < ub[2]):
            out.add(("uv_overlap",))
    return out


def tile_case(case):
    """would the tiles take this case (even ld, aligned bases)?"""
    return case.ld % 2 == 0 and not case.shift


def _ys(rng, ny, k):
    """row extents that cycle through one row, two rows, ys = 2, ye = ny - 1 and random ones"""
    kind = k % 6
    if kind == 0:
        return 1, 1                                     # (0-based) one row at ys = 2
    if kind == 1:
        return ny - 2, ny - 2                           # one row at ye = ny - 1
    if kind == 2:
        return 1, min(2, ny - 2)                        # two rows from ys = 2 (one if ny = 3)
    if kind == 3:
        return max(ny - 3, 1), ny - 2                   # two rows ending at ny - 1
    if kind == 4:
        return 1, ny - 2
    y0 = int(rng.integers(1, ny - 1))
    return y0, int(rng.integers(y0, ny - 1))


def _fixed(rng):
    C_ = []
    k = 0

    def add(ld, ny, tb, ub=None, vb=None, shift=0):
        c = Case(ld, ny, tb, tb if ub is None else ub, tb if vb is None else vb, shift)
        C_.append(c)

    # x0 even / odd x x1 even / odd, first chunk 0, 1, 7 chunks past its 128-byte anchor
    for off in (0, 1, 7):
        for p0 in (0, 1):
            for p1 in (0, 1):
                cf = 8 * (1 + k % 3)
                x0 = 2 * (cf + off) + p0
                x1 = 2 * (cf + 40 + 3 * off) + p1
                ld = x1 + 2 + x1 % 2 + 2 * (k % 5)       # even: the tiles
                ny = 6 + k % 7
                y0, y1 = _ys(rng, ny, k)
                add(ld, ny, _b(x0, x1, y0, y1))
                k += 1
    # the last column in lanes W-3 .. W-1 of a wave, or lane 0 / 1 of the next, in the first and second wave
    for w in WIDTHS:
        for d in (w - 3, w - 2, w - 1, w, w + 1, 2 * w - 2, 2 * w - 1, 2 * w):
            for p1 in (0, 1):
                off = (0, 1, 3, 7)[k % 4]
                cf = 8 * (k % 3)
                x0 = max(2 * (cf + off) + (k // 4) % 2, 1)
                x1 = 2 * (cf + d) + p1
                ld = x1 + 2 + x1 % 2 + 2 * (k % 4)
                ny = 3 + k % 11
                y0, y1 = _ys(rng, ny, k)
                add(ld, ny, _b(x0, x1, y0, y1))
                k += 1
    # one column (even, odd: the second of its chunk), two columns (in one chunk, across two)
    for x0 in (1, 2, 15, 16, 17, 126, 127):
        ld = 2 * (x0 // 2) + 8
        ny = 5 + x0 % 4
        y0, y1 = _ys(rng, ny, k)
        add(ld, ny, _b(x0, x0, y0, y1))
        add(ld, ny, _b(x0, x0 + 1, y0, y1))
        k += 1
    # the box touches the ring on all four sides: one wave, several waves
    for ld, ny in ((8, 3), (64, 5), (130, 20), (1000, 7), (1026, 12), (1090, 4)):
        add(ld, ny, (2, ld - 1, 2, ny - 1))
    # U and V boxes that differ in every edge and overlap in part; a sub-box whose first chunk is lane 0 of wave 1 / 2
    for w in WIDTHS:
        for kk in (1, 2):
            cf = 8
            x0 = 2 * cf + 1
            xv0 = 2 * (cf + kk * w)
            ld = xv0 + 2 * w + 40
            ny = 9 + kk
            add(ld, ny, _b(x0, xv0 + 5, 1, ny - 3), _b(x0, xv0 + 5, 1, ny - 3), _b(xv0, ld - 3, 2, ny - 2))
            add(ld, ny, _b(x0 + 2, ld - 2, 1, ny - 2), _b(x0 + 2, xv0 + 40, 2, ny - 2), _b(xv0, ld - 2, 1, ny - 3))
    add(300, 40, (37, 250, 5, 36), (40, 250, 5, 30), (33, 251, 7, 39))
    add(1100, 21, (2, 1099, 2, 20), (129, 900, 3, 20), (2, 1000, 2, 15))
    # empty boxes
    add(200, 30, (2, 199, 2, 29), (2, 199, 2, 29), EMPTY)
    add(200, 30, (2, 199, 2, 29), EMPTY, (2, 199, 2, 29))
    add(1000, 11, (30, 700, 3, 9), EMPTY, (30, 700, 3, 9))
    add(200, 30, EMPTY, EMPTY, EMPTY)
    return C_


def _rand_box(rng, ld, ny):
    if rng.random() < 0.04:
        return EMPTY
    x0 = int(rng.integers(1, ld - 1))
    x1 = int(rng.integers(x0, ld - 1)) if rng.random() < 0.7 else ld - 2
    y0 = int(rng.integers(1, ny - 1))
    y1 = int(rng.integers(y0, ny - 1))
    return _b(x0, x1, y0, y1)


def _random(rng, n):
    C_ = []
    for _ in range(n):
        ld = int(rng.integers(8, 1101))
        ld = ld + ld % 2 if rng.random() < 0.8 else ld | 1      # mostly even (the tiles), some odd (the one-cell forms)
        ny = int(rng.integers(3, 41))
        shift = int(rng.random() < 0.125)
        tb = _rand_box(rng, ld, ny)
        r = rng.random()
        if r < 0.5:
            ub = vb = tb                                 # one box: the step tile
        elif r < 0.75:
            ub, vb = _rand_box(rng, ld, ny), _rand_box(rng, ld, ny)
        else:
            ub, vb = tb, _rand_box(rng, ld, ny)
        C_.append(Case(ld, ny, tb, ub, vb, shift))
    return C_


def cases(seed=20261016, n_random=72):
    """the fixed edge placements, then n_random random cases; deterministic for a seed"""
    rng = np.random.default_rng(seed)
    return _fixed(rng) + _random(rng, n_random)


N_FIXED = len(_fixed(np.random.default_rng(0)))


def case_id(k, c):
    return f"{'f' if k < N_FIXED else 'r'}{k}-ld{c.ld}x{c.ny}{'-s' if c.shift else ''}"
