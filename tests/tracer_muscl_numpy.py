"""Independent CPU evaluation of the second-order limited tracer transport rule of DESIGN.md section 6.11.

TEST INFRASTRUCTURE.  The reference holds no such loop, so its specification is frozen in DESIGN.md section 6.11 and
nothing in the reference can pin it.  Two evaluations are written here from that text, separately:
  * whole-array numpy expressions (`tracer_step_muscl`): the slopes sx, sy of every cell of the array from copies padded by
    one cell on every side -- the mask with 0, the tracer with its own edge values, which the mask then switches off -- and
    the update over shifted views of the box;
  * a plain scalar loop (`tracer_step_muscl_scalar`), one cell at a time, line by line, that asks for T(i, j) through a
    function returning 0 outside the array and reads a tracer value only behind that test.
Neither ever forms a negative index: numpy would wrap it to the other end of the array.  Both round every operation in
double precision in the association order the parentheses give, both choose with selects -- np.where, if / else -- and never
blend, and MC's comparisons are comparisons, not fmin / fmax.  They are required to agree with each other, and with the GPU,
bit for bit.

Index convention, arguments and what is left unwritten: tests/tracer_numpy.py.
"""
import numpy as np

from tracer_numpy import _div, _view, same  # noqa: F401  (same: for the tests that import this module alone)


def _mc(a, b):
    """MC(a, b) on arrays"""
    a2 = 2.0 * np.abs(a)
    b2 = 2.0 * np.abs(b)
    m = 0.5 * np.abs(a + b)
    lo = np.where(a2 < b2, a2, b2)
    lo = np.where(m < lo, m, lo)
    return np.where((a > 0.0) & (b > 0.0), lo, np.where((a < 0.0) & (b < 0.0), -lo, 0.0))


def slopes(tmask, c):
    """(sx, sy) of every cell of the array; T = 0 outside it"""
    T = np.pad(tmask, 1, mode="constant", constant_values=0)
    C = np.pad(c, 1, mode="edge")
    mid = (slice(1, -1), slice(1, -1))
    west, east = (slice(1, -1), slice(0, -2)), (slice(1, -1), slice(2, None))
    south, north = (slice(0, -2), slice(1, -1)), (slice(2, None), slice(1, -1))
    with np.errstate(all="ignore"):
        sx = np.where((T[mid] > 0) & (T[west] != 0) & (T[east] != 0), _mc(C[mid] - C[west], C[east] - C[mid]), 0.0)
        sy = np.where((T[mid] > 0) & (T[south] != 0) & (T[north] != 0), _mc(C[mid] - C[south], C[north] - C[mid]), 0.0)
    return sx, sy


def tracer_step_muscl(rdt, box, tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, ssha, c_in, c_out):
    """DESIGN.md section 6.11 on whole arrays; the argument order of dlesm_tracer_step_muscl_f64"""
    xs, xe, ys, ye = box
    if xe < xs or ye < ys:
        return
    assert len(c_in) == len(c_out)
    assert xs >= 2 and ys >= 2 and xe <= tmask.shape[1] - 1 and ye <= tmask.shape[0] - 1      # the ring: no view wraps
    rdt = float(rdt)
    S = _view(box)
    T = tmask
    wet = S(T) > 0
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
            ce = np.where(r1 >= 0.0, S(c) + 0.5 * S(sx), S(c, 1, 0) - 0.5 * S(sx, 1, 0))
            cw = np.where(r2 >= 0.0, S(c, -1, 0) + 0.5 * S(sx, -1, 0), S(c) - 0.5 * S(sx))
            cn = np.where(r3 >= 0.0, S(c) + 0.5 * S(sy), S(c, 0, 1) - 0.5 * S(sy, 0, 1))
            cs = np.where(r4 >= 0.0, S(c, 0, -1) + 0.5 * S(sy, 0, -1), S(c) - 0.5 * S(sy))
            F1 = np.where(S(T, 1, 0) != 0, r1 * ce, 0.0)
            F2 = np.where(S(T, -1, 0) != 0, r2 * cw, 0.0)
            F3 = np.where(S(T, 0, 1) != 0, r3 * cn, 0.0)
            F4 = np.where(S(T, 0, -1) != 0, r4 * cs, 0.0)
            val = (h_old * S(c) + (((F2 - F1) + F4) - F3) * q) / h_new
            S(out)[wet] = val[wet]


def _mc_scalar(a, b):
    a2 = 2.0 * abs(a)
    b2 = 2.0 * abs(b)
    m = 0.5 * abs(a + b)
    lo = a2 if a2 < b2 else b2
    lo = m if m < lo else lo
    if a > 0.0 and b > 0.0:
        return lo
    if a < 0.0 and b < 0.0:
        return -lo
    return 0.0


def tracer_step_muscl_scalar(rdt, box, tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, ssha, c_in, c_out):
    """the same rule, one cell at a time; i, j are 0-based here"""
    xs, xe, ys, ye = box
    rdt = float(rdt)
    ny, ld = tmask.shape

    def T(i, j):
        return int(tmask[j, i]) if 0 <= i < ld and 0 <= j < ny else 0

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
            for c, out in zip(c_in, c_out):
                here = float(c[j, i])
                if r1 >= 0.0:
                    ce = here + 0.5 * sx(c, i, j)
                else:
                    ce = float(c[j, i + 1]) - 0.5 * sx(c, i + 1, j)
                if r2 >= 0.0:
                    cw = float(c[j, i - 1]) + 0.5 * sx(c, i - 1, j)
                else:
                    cw = here - 0.5 * sx(c, i, j)
                if r3 >= 0.0:
                    cn = here + 0.5 * sy(c, i, j)
                else:
                    cn = float(c[j + 1, i]) - 0.5 * sy(c, i, j + 1)
                if r4 >= 0.0:
                    cs = float(c[j - 1, i]) + 0.5 * sy(c, i, j - 1)
                else:
                    cs = here - 0.5 * sy(c, i, j)
                F1 = r1 * ce if T(i + 1, j) != 0 else 0.0
                F2 = r2 * cw if T(i - 1, j) != 0 else 0.0
                F3 = r3 * cn if T(i, j + 1) != 0 else 0.0
                F4 = r4 * cs if T(i, j - 1) != 0 else 0.0
                out[j, i] = _div(h_old * here + (((F2 - F1) + F4) - F3) * q, h_new)
