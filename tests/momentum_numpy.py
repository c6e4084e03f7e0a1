"""Independent CPU evaluation of the NEMOLite2D-class momentum and sea-surface-height interpolation kernels of
DESIGN.md section 6.5.

TEST INFRASTRUCTURE.  The reference holds none of these loops, so their specification is frozen in DESIGN.md section 6.5
and nothing in the reference can pin it.  Two evaluations are written here from that text, separately:
  * whole-array numpy expressions over shifted views of the box (`momentum_u`, `momentum_v`, `momentum`, `next_sshu`,
    `next_sshv`), applied in bands of rows so that a 4096^2 case fits in host memory;
  * a plain scalar loop (`*_scalar`), one cell at a time, line by line.
Both round every operation in double precision in the association order the parentheses give: numpy's elementwise
float64 operations never contract a*b+c, as the kernels are built with -ffp-contract=off.  They are required to agree
with each other, and with the GPU, bit for bit.

Index convention: arrays are (ny, ld) C-order, Fortran element (i, j) = arr[j-1, i-1]; boxes are 1-based inclusive
(xstart, xstop, ystart, ystop).  `grid` is any object with the attributes tmask (int32), dx_t, dy_t, dx_u, dy_u, dx_v,
dy_v, area_u, area_v, fcor_u, fcor_v; `prm` any object with rdt, cbfr, visc, g.  A cell the rule does not write keeps
its content; nothing outside the box is written.
"""
import math
import os
from types import SimpleNamespace

import numpy as np

GRID_ARRAYS = ("tmask", "dx_t", "dy_t", "dx_u", "dy_u", "dx_v", "dy_v", "area_u", "area_v", "fcor_u", "fcor_v")
BAND_ROWS = 256


def params(rdt, cbfr, visc, g):
    return SimpleNamespace(rdt=float(rdt), cbfr=float(cbfr), visc=float(visc), g=float(g))


def _s(x):
    """s(x) = copysign(0.5, x): Fortran SIGN(0.5, x) with signed zeros"""
    return np.copysign(0.5, x)


def _bands(box):
    xs, xe, ys, ye = box
    for b0 in range(ys, ye + 1, BAND_ROWS):
        yield (xs, xe, b0, min(ye, b0 + BAND_ROWS - 1))


def _view(box):
    xs, xe, ys, ye = box

    def S(a, di=0, dj=0):                                 # the box shifted by (di, dj)
        return a[ys - 1 + dj:ye + dj, xs - 1 + di:xe + di]
    return S


def _momentum_u_band(p, G, box, un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, ua):
    S = _view(box)
    T = G.tmask
    wet = (S(T) > 0) & (S(T, 1, 0) > 0)
    sw = (S(T, 0, -1) > 0) & (S(T, 1, -1) > 0)
    nw = (S(T, 0, 1) > 0) & (S(T, 1, 1) > 0)
    u_e = (0.5 * (S(un) + S(un, 1, 0))) * S(G.dy_t, 1, 0)
    depe = S(ht, 1, 0) + S(sshn_t, 1, 0)
    u_w = (0.5 * (S(un) + S(un, -1, 0))) * S(G.dy_t)
    depw = S(ht) + S(sshn_t)
    v_sc = 0.5 * (S(vn, 0, -1) + S(vn, 1, -1))
    v_s = (0.5 * v_sc) * (S(G.dx_v, 0, -1) + S(G.dx_v, 1, -1))
    deps = 0.5 * (((S(hv, 0, -1) + S(sshn_v, 0, -1)) + S(hv, 1, -1)) + S(sshn_v, 1, -1))
    v_nc = 0.5 * (S(vn) + S(vn, 1, 0))
    v_n = (0.5 * v_nc) * (S(G.dx_v) + S(G.dx_v, 1, 0))
    depn = 0.5 * (((S(hv) + S(sshn_v)) + S(hv, 1, 0)) + S(sshn_v, 1, 0))
    uu_w = (0.5 - _s(u_w)) * S(un) + (0.5 + _s(u_w)) * S(un, -1, 0)
    uu_e = (0.5 + _s(u_e)) * S(un) + (0.5 - _s(u_e)) * S(un, 1, 0)
    uu_s = np.where(sw, (0.5 - _s(v_s)) * S(un) + (0.5 + _s(v_s)) * S(un, 0, -1), (0.5 - _s(v_s)) * S(un))
    uu_n = np.where(nw, (0.5 + _s(v_n)) * S(un) + (0.5 - _s(v_n)) * S(un, 0, 1), (0.5 + _s(v_n)) * S(un))
    adv = (((uu_w * u_w) * depw - (uu_e * u_e) * depe) + (uu_s * v_s) * deps) - (uu_n * v_n) * depn
    dudx_e = ((S(un, 1, 0) - S(un)) / S(G.dx_t, 1, 0)) * (S(ht, 1, 0) + S(sshn_t, 1, 0))
    dudx_w = ((S(un) - S(un, -1, 0)) / S(G.dx_t)) * (S(ht) + S(sshn_t))
    dudy_s = np.where(sw, ((S(un) - S(un, 0, -1)) / (S(G.dy_u) + S(G.dy_u, 0, -1))) *
                      (((S(hu) + S(sshn_u)) + S(hu, 0, -1)) + S(sshn_u, 0, -1)), 0.0)
    dudy_n = np.where(nw, ((S(un, 0, 1) - S(un)) / (S(G.dy_u) + S(G.dy_u, 0, 1))) *
                      (((S(hu) + S(sshn_u)) + S(hu, 0, 1)) + S(sshn_u, 0, 1)), 0.0)
    vis = p.visc * ((dudx_e - dudx_w) * S(G.dy_u) + ((dudy_n - dudy_s) * S(G.dx_u)) * 0.5)
    cor = ((0.5 * (S(G.fcor_u) * (v_sc + v_nc))) * S(G.area_u)) * (S(hu) + S(sshn_u))
    hpg = -(((p.g * (S(hu) + S(sshn_u))) * S(G.dy_u)) * (S(sshn_t, 1, 0) - S(sshn_t)))
    val = ((S(un) * (S(hu) + S(sshn_u)) + (p.rdt * (((adv + vis) + cor) + hpg)) / S(G.area_u)) /
           (S(hu) + S(ssha_u))) / (1.0 + p.cbfr * p.rdt)
    S(ua)[wet] = val[wet]


def _momentum_v_band(p, G, box, un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_v, va):
    S = _view(box)
    T = G.tmask
    wet = (S(T) > 0) & (S(T, 0, 1) > 0)
    ww = (S(T, -1, 0) > 0) & (S(T, -1, 1) > 0)
    ew = (S(T, 1, 0) > 0) & (S(T, 1, 1) > 0)
    v_n = (0.5 * (S(vn) + S(vn, 0, 1))) * S(G.dx_t, 0, 1)
    depn = S(ht, 0, 1) + S(sshn_t, 0, 1)
    v_s = (0.5 * (S(vn) + S(vn, 0, -1))) * S(G.dx_t)
    deps = S(ht) + S(sshn_t)
    u_wc = 0.5 * (S(un, -1, 0) + S(un, -1, 1))
    u_w = (0.5 * u_wc) * (S(G.dy_u, -1, 0) + S(G.dy_u, -1, 1))
    depw = 0.5 * (((S(hu, -1, 0) + S(sshn_u, -1, 0)) + S(hu, -1, 1)) + S(sshn_u, -1, 1))
    u_ec = 0.5 * (S(un) + S(un, 0, 1))
    u_e = (0.5 * u_ec) * (S(G.dy_u) + S(G.dy_u, 0, 1))
    depe = 0.5 * (((S(hu) + S(sshn_u)) + S(hu, 0, 1)) + S(sshn_u, 0, 1))
    vv_s = (0.5 - _s(v_s)) * S(vn) + (0.5 + _s(v_s)) * S(vn, 0, -1)
    vv_n = (0.5 + _s(v_n)) * S(vn) + (0.5 - _s(v_n)) * S(vn, 0, 1)
    vv_w = np.where(ww, (0.5 - _s(u_w)) * S(vn) + (0.5 + _s(u_w)) * S(vn, -1, 0), (0.5 - _s(u_w)) * S(vn))
    vv_e = np.where(ew, (0.5 + _s(u_e)) * S(vn) + (0.5 - _s(u_e)) * S(vn, 1, 0), (0.5 + _s(u_e)) * S(vn))
    adv = (((vv_w * u_w) * depw - (vv_e * u_e) * depe) + (vv_s * v_s) * deps) - (vv_n * v_n) * depn
    dvdy_n = ((S(vn, 0, 1) - S(vn)) / S(G.dy_t, 0, 1)) * (S(ht, 0, 1) + S(sshn_t, 0, 1))
    dvdy_s = ((S(vn) - S(vn, 0, -1)) / S(G.dy_t)) * (S(ht) + S(sshn_t))
    dvdx_w = np.where(ww, ((S(vn) - S(vn, -1, 0)) / (S(G.dx_v) + S(G.dx_v, -1, 0))) *
                      (((S(hv) + S(sshn_v)) + S(hv, -1, 0)) + S(sshn_v, -1, 0)), 0.0)
    dvdx_e = np.where(ew, ((S(vn, 1, 0) - S(vn)) / (S(G.dx_v) + S(G.dx_v, 1, 0))) *
                      (((S(hv) + S(sshn_v)) + S(hv, 1, 0)) + S(sshn_v, 1, 0)), 0.0)
    vis = p.visc * ((dvdy_n - dvdy_s) * S(G.dx_v) + ((dvdx_e - dvdx_w) * S(G.dy_v)) * 0.5)
    cor = -(((0.5 * (S(G.fcor_v) * (u_ec + u_wc))) * S(G.area_v)) * (S(hv) + S(sshn_v)))
    hpg = -(((p.g * (S(hv) + S(sshn_v))) * S(G.dx_v)) * (S(sshn_t, 0, 1) - S(sshn_t)))
    val = ((S(vn) * (S(hv) + S(sshn_v)) + (p.rdt * (((adv + vis) + cor) + hpg)) / S(G.area_v)) /
           (S(hv) + S(ssha_v))) / (1.0 + p.cbfr * p.rdt)
    S(va)[wet] = val[wet]


def _next_ssh_band(box, di, dj, tmask, area_t, area_x, sshn_t, out):
    S = _view(box)
    t0, t1 = S(tmask).astype(np.int64), S(tmask, di, dj).astype(np.int64)
    both = (0.5 * (S(area_t) * S(sshn_t) + S(area_t, di, dj) * S(sshn_t, di, dj))) / S(area_x)
    val = np.where(t0 * t1 > 0, both, np.where(t0 <= 0, S(sshn_t, di, dj), S(sshn_t)))
    w = t0 + t1 > 0
    S(out)[w] = val[w]


def _banded(fn, box, *args):
    """fn over the box in bands of rows, in a thread pool (numpy releases the GIL; bands write disjoint rows)"""
    if box[1] < box[0] or box[3] < box[2]:
        return
    from concurrent.futures import ThreadPoolExecutor

    def band(b):
        with np.errstate(all="ignore"):                   # dry cells may divide by zero; their values are discarded
            fn(b, *args)
    bands = list(_bands(box))
    if len(bands) == 1:
        band(bands[0])
        return
    with ThreadPoolExecutor(min(len(bands), os.cpu_count() or 1)) as ex:
        list(ex.map(band, bands))


def momentum_u(prm, grid, box, un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, ua):
    """momentum_u over the box: ua(i,j) where T(i,j) > 0 and T(i+1,j) > 0"""
    _banded(lambda b, *a: _momentum_u_band(prm, grid, b, *a), box, un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, ua)


def momentum_v(prm, grid, box, un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_v, va):
    """momentum_v over the box: va(i,j) where T(i,j) > 0 and T(i,j+1) > 0"""
    _banded(lambda b, *a: _momentum_v_band(prm, grid, b, *a), box, un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_v, va)


def momentum(prm, grid, ubox, vbox, un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, ssha_v, ua, va):
    """the fused entry: momentum_u over ubox, then momentum_v over vbox"""
    momentum_u(prm, grid, ubox, un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, ua)
    momentum_v(prm, grid, vbox, un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_v, va)


def next_sshu(box, tmask, area_t, area_u, sshn_t, sshn_u):
    _banded(lambda b, *a: _next_ssh_band(b, 1, 0, *a), box, tmask, area_t, area_u, sshn_t, sshn_u)


def next_sshv(box, tmask, area_t, area_v, sshn_t, sshn_v):
    _banded(lambda b, *a: _next_ssh_band(b, 0, 1, *a), box, tmask, area_t, area_v, sshn_t, sshn_v)


# ---- the scalar restatement: one cell at a time, numpy float64 scalars (IEEE division by zero instead of an exception)
def _cells(box):
    xs, xe, ys, ye = box
    for j in range(ys, ye + 1):
        for i in range(xs, xe + 1):
            yield i, j


def _sg(x):
    return np.float64(math.copysign(0.5, float(x)))


def momentum_u_scalar(prm, G, box, un_, vn_, ht_, sshn_t_, hu_, sshn_u_, hv_, sshn_v_, ssha_u_, ua):
    f64 = np.float64
    rdt, cbfr, visc, g = f64(prm.rdt), f64(prm.cbfr), f64(prm.visc), f64(prm.g)

    def at(a):
        return lambda i, j: a[j - 1, i - 1]
    T = at(G.tmask)
    un, vn, ht, sshn_t, hu, sshn_u = at(un_), at(vn_), at(ht_), at(sshn_t_), at(hu_), at(sshn_u_)
    hv, sshn_v, ssha_u = at(hv_), at(sshn_v_), at(ssha_u_)
    dx_t, dy_t, dx_u, dy_u, dx_v = at(G.dx_t), at(G.dy_t), at(G.dx_u), at(G.dy_u), at(G.dx_v)
    area_u, fcor_u = at(G.area_u), at(G.fcor_u)
    with np.errstate(all="ignore"):
        for i, j in _cells(box):
            if not (T(i, j) > 0 and T(i + 1, j) > 0):
                continue
            sw = T(i, j - 1) > 0 and T(i + 1, j - 1) > 0
            nw = T(i, j + 1) > 0 and T(i + 1, j + 1) > 0
            u_e = (0.5 * (un(i, j) + un(i + 1, j))) * dy_t(i + 1, j)
            depe = ht(i + 1, j) + sshn_t(i + 1, j)
            u_w = (0.5 * (un(i, j) + un(i - 1, j))) * dy_t(i, j)
            depw = ht(i, j) + sshn_t(i, j)
            v_sc = 0.5 * (vn(i, j - 1) + vn(i + 1, j - 1))
            v_s = (0.5 * v_sc) * (dx_v(i, j - 1) + dx_v(i + 1, j - 1))
            deps = 0.5 * (((hv(i, j - 1) + sshn_v(i, j - 1)) + hv(i + 1, j - 1)) + sshn_v(i + 1, j - 1))
            v_nc = 0.5 * (vn(i, j) + vn(i + 1, j))
            v_n = (0.5 * v_nc) * (dx_v(i, j) + dx_v(i + 1, j))
            depn = 0.5 * (((hv(i, j) + sshn_v(i, j)) + hv(i + 1, j)) + sshn_v(i + 1, j))
            uu_w = (0.5 - _sg(u_w)) * un(i, j) + (0.5 + _sg(u_w)) * un(i - 1, j)
            uu_e = (0.5 + _sg(u_e)) * un(i, j) + (0.5 - _sg(u_e)) * un(i + 1, j)
            if sw:
                uu_s = (0.5 - _sg(v_s)) * un(i, j) + (0.5 + _sg(v_s)) * un(i, j - 1)
            else:
                uu_s = (0.5 - _sg(v_s)) * un(i, j)
            if nw:
                uu_n = (0.5 + _sg(v_n)) * un(i, j) + (0.5 - _sg(v_n)) * un(i, j + 1)
            else:
                uu_n = (0.5 + _sg(v_n)) * un(i, j)
            adv = (((uu_w * u_w) * depw - (uu_e * u_e) * depe) + (uu_s * v_s) * deps) - (uu_n * v_n) * depn
            dudx_e = ((un(i + 1, j) - un(i, j)) / dx_t(i + 1, j)) * (ht(i + 1, j) + sshn_t(i + 1, j))
            dudx_w = ((un(i, j) - un(i - 1, j)) / dx_t(i, j)) * (ht(i, j) + sshn_t(i, j))
            dudy_s = f64(0.0)
            if sw:
                dudy_s = ((un(i, j) - un(i, j - 1)) / (dy_u(i, j) + dy_u(i, j - 1))) * \
                    (((hu(i, j) + sshn_u(i, j)) + hu(i, j - 1)) + sshn_u(i, j - 1))
            dudy_n = f64(0.0)
            if nw:
                dudy_n = ((un(i, j + 1) - un(i, j)) / (dy_u(i, j) + dy_u(i, j + 1))) * \
                    (((hu(i, j) + sshn_u(i, j)) + hu(i, j + 1)) + sshn_u(i, j + 1))
            vis = visc * ((dudx_e - dudx_w) * dy_u(i, j) + ((dudy_n - dudy_s) * dx_u(i, j)) * 0.5)
            cor = ((0.5 * (fcor_u(i, j) * (v_sc + v_nc))) * area_u(i, j)) * (hu(i, j) + sshn_u(i, j))
            hpg = -(((g * (hu(i, j) + sshn_u(i, j))) * dy_u(i, j)) * (sshn_t(i + 1, j) - sshn_t(i, j)))
            ua[j - 1, i - 1] = ((un(i, j) * (hu(i, j) + sshn_u(i, j)) + (rdt * (((adv + vis) + cor) + hpg)) / area_u(i, j)) /
                                (hu(i, j) + ssha_u(i, j))) / (1.0 + cbfr * rdt)


def momentum_v_scalar(prm, G, box, un_, vn_, ht_, sshn_t_, hu_, sshn_u_, hv_, sshn_v_, ssha_v_, va):
    f64 = np.float64
    rdt, cbfr, visc, g = f64(prm.rdt), f64(prm.cbfr), f64(prm.visc), f64(prm.g)

    def at(a):
        return lambda i, j: a[j - 1, i - 1]
    T = at(G.tmask)
    un, vn, ht, sshn_t, hu, sshn_u = at(un_), at(vn_), at(ht_), at(sshn_t_), at(hu_), at(sshn_u_)
    hv, sshn_v, ssha_v = at(hv_), at(sshn_v_), at(ssha_v_)
    dx_t, dy_t, dy_u, dx_v, dy_v = at(G.dx_t), at(G.dy_t), at(G.dy_u), at(G.dx_v), at(G.dy_v)
    area_v, fcor_v = at(G.area_v), at(G.fcor_v)
    with np.errstate(all="ignore"):
        for i, j in _cells(box):
            if not (T(i, j) > 0 and T(i, j + 1) > 0):
                continue
            ww = T(i - 1, j) > 0 and T(i - 1, j + 1) > 0
            ew = T(i + 1, j) > 0 and T(i + 1, j + 1) > 0
            v_n = (0.5 * (vn(i, j) + vn(i, j + 1))) * dx_t(i, j + 1)
            depn = ht(i, j + 1) + sshn_t(i, j + 1)
            v_s = (0.5 * (vn(i, j) + vn(i, j - 1))) * dx_t(i, j)
            deps = ht(i, j) + sshn_t(i, j)
            u_wc = 0.5 * (un(i - 1, j) + un(i - 1, j + 1))
            u_w = (0.5 * u_wc) * (dy_u(i - 1, j) + dy_u(i - 1, j + 1))
            depw = 0.5 * (((hu(i - 1, j) + sshn_u(i - 1, j)) + hu(i - 1, j + 1)) + sshn_u(i - 1, j + 1))
            u_ec = 0.5 * (un(i, j) + un(i, j + 1))
            u_e = (0.5 * u_ec) * (dy_u(i, j) + dy_u(i, j + 1))
            depe = 0.5 * (((hu(i, j) + sshn_u(i, j)) + hu(i, j + 1)) + sshn_u(i, j + 1))
            vv_s = (0.5 - _sg(v_s)) * vn(i, j) + (0.5 + _sg(v_s)) * vn(i, j - 1)
            vv_n = (0.5 + _sg(v_n)) * vn(i, j) + (0.5 - _sg(v_n)) * vn(i, j + 1)
            if ww:
                vv_w = (0.5 - _sg(u_w)) * vn(i, j) + (0.5 + _sg(u_w)) * vn(i - 1, j)
            else:
                vv_w = (0.5 - _sg(u_w)) * vn(i, j)
            if ew:
                vv_e = (0.5 + _sg(u_e)) * vn(i, j) + (0.5 - _sg(u_e)) * vn(i + 1, j)
            else:
                vv_e = (0.5 + _sg(u_e)) * vn(i, j)
            adv = (((vv_w * u_w) * depw - (vv_e * u_e) * depe) + (vv_s * v_s) * deps) - (vv_n * v_n) * depn
            dvdy_n = ((vn(i, j + 1) - vn(i, j)) / dy_t(i, j + 1)) * (ht(i, j + 1) + sshn_t(i, j + 1))
            dvdy_s = ((vn(i, j) - vn(i, j - 1)) / dy_t(i, j)) * (ht(i, j) + sshn_t(i, j))
            dvdx_w = f64(0.0)
            if ww:
                dvdx_w = ((vn(i, j) - vn(i - 1, j)) / (dx_v(i, j) + dx_v(i - 1, j))) * \
                    (((hv(i, j) + sshn_v(i, j)) + hv(i - 1, j)) + sshn_v(i - 1, j))
            dvdx_e = f64(0.0)
            if ew:
                dvdx_e = ((vn(i + 1, j) - vn(i, j)) / (dx_v(i, j) + dx_v(i + 1, j))) * \
                    (((hv(i, j) + sshn_v(i, j)) + hv(i + 1, j)) + sshn_v(i + 1, j))
            vis = visc * ((dvdy_n - dvdy_s) * dx_v(i, j) + ((dvdx_e - dvdx_w) * dy_v(i, j)) * 0.5)
            cor = -(((0.5 * (fcor_v(i, j) * (u_ec + u_wc))) * area_v(i, j)) * (hv(i, j) + sshn_v(i, j)))
            hpg = -(((g * (hv(i, j) + sshn_v(i, j))) * dx_v(i, j)) * (sshn_t(i, j + 1) - sshn_t(i, j)))
            va[j - 1, i - 1] = ((vn(i, j) * (hv(i, j) + sshn_v(i, j)) + (rdt * (((adv + vis) + cor) + hpg)) / area_v(i, j)) /
                                (hv(i, j) + ssha_v(i, j))) / (1.0 + cbfr * rdt)


def _next_ssh_scalar(box, di, dj, tmask, area_t, area_x, sshn_t, out):
    with np.errstate(all="ignore"):
        for i, j in _cells(box):
            t0, t1 = int(tmask[j - 1, i - 1]), int(tmask[j - 1 + dj, i - 1 + di])
            if t0 + t1 <= 0:
                continue
            if t0 * t1 > 0:
                out[j - 1, i - 1] = (0.5 * (area_t[j - 1, i - 1] * sshn_t[j - 1, i - 1] +
                                            area_t[j - 1 + dj, i - 1 + di] * sshn_t[j - 1 + dj, i - 1 + di])) / area_x[j - 1, i - 1]
            elif t0 <= 0:
                out[j - 1, i - 1] = sshn_t[j - 1 + dj, i - 1 + di]
            else:
                out[j - 1, i - 1] = sshn_t[j - 1, i - 1]


def next_sshu_scalar(box, tmask, area_t, area_u, sshn_t, sshn_u):
    _next_ssh_scalar(box, 1, 0, tmask, area_t, area_u, sshn_t, sshn_u)


def next_sshv_scalar(box, tmask, area_t, area_v, sshn_t, sshn_v):
    _next_ssh_scalar(box, 0, 1, tmask, area_t, area_v, sshn_t, sshn_v)


def coriolis(gphi, omega, d2r):
    """fcor = (2*omega) * sin(gphi*d2r), evaluated on the host (the PSy layers' one-time computation)"""
    return (2.0 * omega) * np.sin(gphi * d2r)


def same(a, b):
    """bit-for-bit equality, any NaN equal to any NaN (the sign and payload of a generated NaN are not specified)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))
