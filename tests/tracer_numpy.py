"""Independent CPU evaluation of the tracer transport rule of DESIGN.md section 6.10.

TEST INFRASTRUCTURE.  The reference holds no such loop, so its specification is frozen in DESIGN.md section 6.10 and
nothing in the reference can pin it.  Two evaluations are written here from that text, separately:
  * whole-array numpy expressions over shifted views of the box (`tracer_step`), applied in bands of rows so that a
    4096^2 case fits in host memory;
  * a plain scalar loop (`tracer_step_scalar`), one cell at a time, line by line.
Both round every operation in double precision in the association order the parentheses give (numpy's elementwise float64
operations never contract a*b+c), both choose with selects -- np.where, if / else -- and never blend, so that what a land
cell or a face that touches land holds cannot reach a written cell.  They are required to agree with each other, and with
the GPU, bit for bit.

Index convention: arrays are (ny, ld) C-order, Fortran element (i, j) = arr[j-1, i-1]; boxes are 1-based inclusive
(xstart, xstop, ystart, ystop) with a one-cell ring inside the arrays.  c_in and c_out are lists of arrays.  A cell the rule
does not write (tmask <= 0, or outside the box) keeps its content.
"""
import numpy as np

BAND_ROWS = 256


def same(a, b):
    """bit-for-bit equality of two float64 arrays (NaN payloads and signed zeros included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def _view(box):
    xs, xe, ys, ye = box

    def S(a, di=0, dj=0):                                 # the box shifted by (di, dj)
        return a[ys - 1 + dj:ye + dj, xs - 1 + di:xe + di]
    return S


def _band(rdt, box, tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, ssha, c_in, c_out):
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
            F1 = np.where(S(T, 1, 0) != 0, r1 * np.where(r1 >= 0.0, S(c), S(c, 1, 0)), 0.0)
            F2 = np.where(S(T, -1, 0) != 0, r2 * np.where(r2 >= 0.0, S(c, -1, 0), S(c)), 0.0)
            F3 = np.where(S(T, 0, 1) != 0, r3 * np.where(r3 >= 0.0, S(c), S(c, 0, 1)), 0.0)
            F4 = np.where(S(T, 0, -1) != 0, r4 * np.where(r4 >= 0.0, S(c, 0, -1), S(c)), 0.0)
            val = (h_old * S(c) + (((F2 - F1) + F4) - F3) * q) / h_new
            S(out)[wet] = val[wet]


def tracer_step(rdt, box, tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, ssha, c_in, c_out):
    """DESIGN.md section 6.10 on whole arrays; the argument order of dlesm_tracer_step_f64"""
    xs, xe, ys, ye = box
    if xe < xs or ye < ys:
        return
    assert len(c_in) == len(c_out)
    for b0 in range(ys, ye + 1, BAND_ROWS):
        _band(float(rdt), (xs, xe, b0, min(ye, b0 + BAND_ROWS - 1)), tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v,
              ssha, c_in, c_out)


def _div(a, b):
    """IEEE division of two doubles (Python raises on a zero divisor)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def tracer_step_scalar(rdt, box, tmask, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, ssha, c_in, c_out):
    """the same rule, one cell at a time"""
    xs, xe, ys, ye = box
    rdt = float(rdt)
    for j in range(ys - 1, ye):
        for i in range(xs - 1, xe):
            if tmask[j, i] <= 0:
                continue
            r1 = (float(sshn_u[j, i]) + float(hu[j, i])) * float(un[j, i])
            r2 = (float(sshn_u[j, i - 1]) + float(hu[j, i - 1])) * float(un[j, i - 1])
            r3 = (float(sshn_v[j, i]) + float(hv[j, i])) * float(vn[j, i])
            r4 = (float(sshn_v[j - 1, i]) + float(hv[j - 1, i])) * float(vn[j - 1, i])
            q = _div(rdt, area_t[j, i])
            h_old = float(ht[j, i]) + float(sshn_t[j, i])
            h_new = float(ht[j, i]) + float(ssha[j, i])
            for c, out in zip(c_in, c_out):
                here = float(c[j, i])
                if tmask[j, i + 1] != 0:
                    F1 = r1 * (here if r1 >= 0.0 else float(c[j, i + 1]))
                else:
                    F1 = 0.0
                if tmask[j, i - 1] != 0:
                    F2 = r2 * (float(c[j, i - 1]) if r2 >= 0.0 else here)
                else:
                    F2 = 0.0
                if tmask[j + 1, i] != 0:
                    F3 = r3 * (here if r3 >= 0.0 else float(c[j + 1, i]))
                else:
                    F3 = 0.0
                if tmask[j - 1, i] != 0:
                    F4 = r4 * (float(c[j - 1, i]) if r4 >= 0.0 else here)
                else:
                    F4 = 0.0
                out[j, i] = _div(h_old * here + (((F2 - F1) + F4) - F3) * q, h_new)
