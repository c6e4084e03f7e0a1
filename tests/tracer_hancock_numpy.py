"""Independent CPU evaluation of the time-centred (Hancock) limited tracer transport rule of DESIGN.md section 6.12.

TEST INFRASTRUCTURE.  The reference holds no such loop, so its specification is frozen in DESIGN.md section 6.12 and
nothing in the reference can pin it.  Two evaluations are written here from that text, separately:
  * whole-array numpy expressions (`tracer_step_hancock`): the weight w of every cell of the array in one expression, the
    slopes of section 6.11 from tracer_muscl_numpy's padded copies, and the Courant numbers, factors and update over
    shifted views of the box;
  * a plain scalar loop (`tracer_step_hancock_scalar`), one cell at a time, line by line, that asks for T(i, j) through a
    function returning 0 outside the array, reads a tracer value only behind that test, and evaluates w only in the cell
    and its four neighbours, which the box's ring keeps inside the array.
Neither ever forms a negative index: numpy would wrap it to the other end of the array.  Both round every operation in
double precision in the association order the parentheses give, both choose with selects -- np.where, if / else -- and never
blend; the factor's two comparisons are comparisons (a NaN Courant number fails them and gives 0.0).  They are required to
agree with each other, and with the GPU, bit for bit.

Index convention, arguments and what is left unwritten: tests/tracer_numpy.py.
"""
import numpy as np

from tracer_muscl_numpy import _mc_scalar, slopes
from tracer_numpy import _div, _view, same  # noqa: F401  (same: for the tests that import this module alone)


def weights(rdt, area_t, ht, sshn_t):
    """w of every cell of the array: rdt / (area_t * (ht + sshn_t))"""
    with np.errstate(all="ignore"):
        return float(rdt) / (area_t * (ht + sshn_t))


def _factor(n):
    """g of a face's Courant number n on arrays"""
    with np.errstate(all="ignore"):
        return np.where((n >= 0.0) & (n < 1.0), 0.5 * (1.0 - n), 0.0)


def courant(rdt, box, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v):
    """(n1, n2, n3, n4) over the box: the Courant number of the east, west, north and south face of every cell, each taken
    in the face's upwind cell"""
    S = _view(box)
    w = weights(rdt, area_t, ht, sshn_t)
    with np.errstate(all="ignore"):
        r1 = (S(sshn_u) + S(hu)) * S(un)
        r2 = (S(sshn_u, -1, 0) + S(hu, -1, 0)) * S(un, -1, 0)
        r3 = (S(sshn_v) + S(hv)) * S(vn)
        r4 = (S(sshn_v, 0, -1) + S(hv, 0, -1)) * S(vn, 0, -1)
        n1 = np.abs(r1) * np.where(r1 >= 0.0, S(w), S(w, 1, 0))
        n2 = np.abs(r2) * np.where(r2 >= 0.0, S(w, -1, 0), S(w))
        n3 = np.abs(r3) * np.where(r3 >= 0.0, S(w), S(w, 0, 1))
        n4 = np.abs(r4) * np.where(r4 >= 0.0, S(w, 0, -1), S(w))
    return n1, n2, n3, n4


def face_shares(rdt, box, tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, ssha=None):
    """(share of the faces of the box's wet cells with 0 < n < 1, share with n >= 1): what a test's inputs exercise"""
    wet = _view(box)(tmask) > 0
    with np.errstate(all="ignore"):
        n = np.stack([x[wet] for x in courant(rdt, box, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v)])
        return float(((n > 0.0) & (n < 1.0)).mean()), float((n >= 1.0).mean())


def tracer_step_hancock(rdt, box, tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, ssha, c_in, c_out):
    """DESIGN.md section 6.12 on whole arrays; the argument order of dlesm_tracer_step_hancock_f64"""
    xs, xe, ys, ye = box
    if xe < xs or ye < ys:
        return
    assert len(c_in) == len(c_out)
    assert xs >= 2 and ys >= 2 and xe <= tmask.shape[1] - 1 and ye <= tmask.shape[0] - 1      # the ring: no view wraps
    rdt = float(rdt)
    S = _view(box)
    T = tmask
    wet = S(T) > 0
    n1, n2, n3, n4 = courant(rdt, box, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v)
    g1, g2, g3, g4 = _factor(n1), _factor(n2), _factor(n3), _factor(n4)
    with np.errstate(all="ignore"):
        r1 = (S(sshn_u) + S(hu)) * S(un)
        r2 = (S(sshn_u, -1, 0) + S(hu, -1, 0)) * S(un, -1, 0)
        r3 = (S(sshn_v) + S(hv)) * S(vn)
        r4 = (S(sshn_v, 0, -1) + S(hv, 0, -1)) * S(vn, 0, -1)
        q = rdt / S(area_t)
        h_old = S(ht) + S(sshn_t)
        h_new = S(ht) + S(ssha)
        for c, out in zip(c_in, c_out):
            sx, sy = slopes(T, c)
            ce = np.where(r1 >= 0.0, S(c) + g1 * S(sx), S(c, 1, 0) - g1 * S(sx, 1, 0))
            cw = np.where(r2 >= 0.0, S(c, -1, 0) + g2 * S(sx, -1, 0), S(c) - g2 * S(sx))
            cn = np.where(r3 >= 0.0, S(c) + g3 * S(sy), S(c, 0, 1) - g3 * S(sy, 0, 1))
            cs = np.where(r4 >= 0.0, S(c, 0, -1) + g4 * S(sy, 0, -1), S(c) - g4 * S(sy))
            F1 = np.where(S(T, 1, 0) != 0, r1 * ce, 0.0)
            F2 = np.where(S(T, -1, 0) != 0, r2 * cw, 0.0)
            F3 = np.where(S(T, 0, 1) != 0, r3 * cn, 0.0)
            F4 = np.where(S(T, 0, -1) != 0, r4 * cs, 0.0)
            val = (h_old * S(c) + (((F2 - F1) + F4) - F3) * q) / h_new
            S(out)[wet] = val[wet]


def _factor_scalar(n):
    if n >= 0.0 and n < 1.0:
        return 0.5 * (1.0 - n)
    return 0.0


def tracer_step_hancock_scalar(rdt, box, tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, ssha, c_in, c_out):
    """the same rule, one cell at a time; i, j are 0-based here"""
    xs, xe, ys, ye = box
    rdt = float(rdt)
    ny, ld = tmask.shape

    def T(i, j):
        return int(tmask[j, i]) if 0 <= i < ld and 0 <= j < ny else 0

    def w(i, j):
        assert 0 <= i < ld and 0 <= j < ny
        with np.errstate(all="ignore"):
            return _div(rdt, np.float64(area_t[j, i]) * (np.float64(ht[j, i]) + np.float64(sshn_t[j, i])))

    def sx(c, i, j):
        if T(i, j) > 0 and T(i - 1, j) != 0 and T(i + 1, j) != 0:
            return _mc_scalar(float(c[j, i]) - float(c[j, i - 1]), float(c[j, i + 1]) - float(c[j, i]))
        return 0.0

    def sy(c, i, j):
        if T(i, j) > 0 and T(i, j - 1) != 0 and T(i, j + 1) != 0:
            return _mc_scalar(float(c[j, i]) - float(c[j - 1, i]), float(c[j + 1, i]) - float(c[j, i]))
        return 0.0

    for j in range(ys - 1, ye):
        for i in range(xs - 1, xe):
            if T(i, j) <= 0:
                continue
            assert 1 <= i <= ld - 2 and 1 <= j <= ny - 2          # the ring
            r1 = (float(sshn_u[j, i]) + float(hu[j, i])) * float(un[j, i])
            r2 = (float(sshn_u[j, i - 1]) + float(hu[j, i - 1])) * float(un[j, i - 1])
            r3 = (float(sshn_v[j, i]) + float(hv[j, i])) * float(vn[j, i])
            r4 = (float(sshn_v[j - 1, i]) + float(hv[j - 1, i])) * float(vn[j - 1, i])
            q = _div(rdt, area_t[j, i])
            h_old = float(ht[j, i]) + float(sshn_t[j, i])
            h_new = float(ht[j, i]) + float(ssha[j, i])
            g1 = _factor_scalar(abs(r1) * (w(i, j) if r1 >= 0.0 else w(i + 1, j)))
            g2 = _factor_scalar(abs(r2) * (w(i - 1, j) if r2 >= 0.0 else w(i, j)))
            g3 = _factor_scalar(abs(r3) * (w(i, j) if r3 >= 0.0 else w(i, j + 1)))
            g4 = _factor_scalar(abs(r4) * (w(i, j - 1) if r4 >= 0.0 else w(i, j)))
            for c, out in zip(c_in, c_out):
                here = float(c[j, i])
                if r1 >= 0.0:
                    ce = here + g1 * sx(c, i, j)
                else:
                    ce = float(c[j, i + 1]) - g1 * sx(c, i + 1, j)
                if r2 >= 0.0:
                    cw = float(c[j, i - 1]) + g2 * sx(c, i - 1, j)
                else:
                    cw = here - g2 * sx(c, i, j)
                if r3 >= 0.0:
                    cn = here + g3 * sy(c, i, j)
                else:
                    cn = float(c[j + 1, i]) - g3 * sy(c, i, j + 1)
                if r4 >= 0.0:
                    cs = float(c[j - 1, i]) + g4 * sy(c, i, j - 1)
                else:
                    cs = here - g4 * sy(c, i, j)
                F1 = r1 * ce if T(i + 1, j) != 0 else 0.0
                F2 = r2 * cw if T(i - 1, j) != 0 else 0.0
                F3 = r3 * cn if T(i, j + 1) != 0 else 0.0
                F4 = r4 * cs if T(i, j - 1) != 0 else 0.0
                out[j, i] = _div(h_old * here + (((F2 - F1) + F4) - F3) * q, h_new)
