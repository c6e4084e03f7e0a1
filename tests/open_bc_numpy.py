"""Independent CPU evaluation of the open-boundary kernels of DESIGN.md section 6.6: bc_ssh and the Flather condition on u and v.

TEST INFRASTRUCTURE.  The reference holds none of these loops, so their specification is frozen in DESIGN.md section 6.6.  Two
evaluations are written here from that text, separately:
  * whole-array numpy expressions over shifted views of the box (`bc_ssh`, `flather_u`, `flather_v`, `bc_open`);
  * a plain scalar loop (`*_scalar`), one cell at a time.
Both round every operation in double precision in the order the parentheses give; numpy's sqrt and division are correctly
rounded (IEEE 754).  They are required to agree with each other, and with the GPU, bit for bit.  `refusal` restates which masks
the library's plan refuses.

Index convention as in tests/momentum_numpy.py: arrays are (ny, ld) C-order, Fortran element (i, j) = arr[j-1, i-1]; boxes are
1-based inclusive (xstart, xstop, ystart, ystop).  "Open" is tmask < 0, "wet" tmask > 0.  A cell the rule does not write keeps
its content; nothing outside the box is written.
"""
import math

import numpy as np

from momentum_numpy import params, same  # noqa: F401  (the tests use both from here)


def _empty(box):
    return box[1] < box[0] or box[3] < box[2]


def _view(box):
    xs, xe, ys, ye = box

    def S(a, di=0, dj=0):
        return a[ys - 1 + dj:ye + dj, xs - 1 + di:xe + di]
    return S


def bc_ssh(tbox, tmask, ssh_bc, ssha):
    """ssha = ssh_bc at every open T cell of the box"""
    if _empty(tbox):
        return
    S = _view(tbox)
    S(ssha)[S(tmask) < 0] = ssh_bc


def _flather(box, di, dj, tmask, g, h, sshn_x, sshn_t, x):
    if _empty(box):
        return
    S = _view(box)
    t0, t1 = S(tmask), S(tmask, di, dj)
    first = (t0 < 0) & (t1 > 0)                           # open side west / south: inner face at +1
    second = (t0 > 0) & (t1 < 0)                          # open side east / north: inner face at -1
    with np.errstate(all="ignore"):
        c = np.sqrt(g / S(h))
        v_first = S(x, di, dj) - c * (S(sshn_x, di, dj) - S(sshn_t))
        v_second = S(x, -di, -dj) + c * (S(sshn_x, -di, -dj) - S(sshn_t, di, dj))
    out = S(x)
    out[first] = v_first[first]                           # no inner face is open: every value read above is level n
    out[second] = v_second[second]


def flather_u(prm, ubox, tmask, hu, sshn_u, sshn_t, ua):
    _flather(ubox, 1, 0, tmask, prm.g, hu, sshn_u, sshn_t, ua)


def flather_v(prm, vbox, tmask, hv, sshn_v, sshn_t, va):
    _flather(vbox, 0, 1, tmask, prm.g, hv, sshn_v, sshn_t, va)


def bc_open(prm, tbox, ubox, vbox, tmask, ssh_bc, hu, sshn_u, hv, sshn_v, sshn_t, ssha, ua, va):
    bc_ssh(tbox, tmask, ssh_bc, ssha)
    flather_u(prm, ubox, tmask, hu, sshn_u, sshn_t, ua)
    flather_v(prm, vbox, tmask, hv, sshn_v, sshn_t, va)


# ---- the scalar restatement
def _cells(box):
    xs, xe, ys, ye = box
    for j in range(ys, ye + 1):
        for i in range(xs, xe + 1):
            yield i, j


def bc_ssh_scalar(tbox, tmask, ssh_bc, ssha):
    for i, j in _cells(tbox):
        if tmask[j - 1, i - 1] < 0:
            ssha[j - 1, i - 1] = ssh_bc


def _flather_scalar(box, di, dj, tmask, g, h, sshn_x, sshn_t, x):
    g = np.float64(g)
    src = x.copy()                                       # the level the rule reads (no inner face is written)
    with np.errstate(all="ignore"):
        for i, j in _cells(box):
            a, b = int(tmask[j - 1, i - 1]), int(tmask[j - 1 + dj, i - 1 + di])
            if a + b <= -1 or (a >= 0 and b >= 0):          # NEMOLite2D's form of the rule (the same on {-1, 0, 1} masks)
                continue
            c = np.sqrt(g / h[j - 1, i - 1])
            if a < 0:                                    # open cell (i,j); inner face (i+di, j+dj)
                ii, jj, oi, oj = i + di, j + dj, i, j
                x[j - 1, i - 1] = src[jj - 1, ii - 1] - c * (sshn_x[jj - 1, ii - 1] - sshn_t[oj - 1, oi - 1])
            else:                                        # open cell (i+di, j+dj); inner face (i-di, j-dj)
                ii, jj, oi, oj = i - di, j - dj, i + di, j + dj
                x[j - 1, i - 1] = src[jj - 1, ii - 1] + c * (sshn_x[jj - 1, ii - 1] - sshn_t[oj - 1, oi - 1])


def flather_u_scalar(prm, ubox, tmask, hu, sshn_u, sshn_t, ua):
    _flather_scalar(ubox, 1, 0, tmask, prm.g, hu, sshn_u, sshn_t, ua)


def flather_v_scalar(prm, vbox, tmask, hv, sshn_v, sshn_t, va):
    _flather_scalar(vbox, 0, 1, tmask, prm.g, hv, sshn_v, sshn_t, va)


# ---- which masks the plan refuses, and a repair for random ones
def _open(a, b):
    return (a < 0 and b > 0) or (a > 0 and b < 0)


def refusal(tmask, ubox, vbox):
    """None if the plan accepts the mask on these boxes, else (kind, i, j, reason) of the first open face it refuses:
    'edge' = the inner face, or one of its T cells, lies outside the array; 'open' = the inner face is itself open"""
    ny, ld = tmask.shape
    for kind, box, di, dj in (("u", ubox, 1, 0), ("v", vbox, 0, 1)):
        if _empty(box):
            continue
        for i, j in _cells(box):
            a, b = int(tmask[j - 1, i - 1]), int(tmask[j - 1 + dj, i - 1 + di])
            if not _open(a, b):
                continue
            ii, jj = (i + di, j + dj) if a < 0 else (i - di, j - dj)
            if ii < 1 or jj < 1 or ii + di > ld or jj + dj > ny:
                return (kind, i, j, "edge")
            if _open(int(tmask[jj - 1, ii - 1]), int(tmask[jj - 1 + dj, ii - 1 + di])):
                return (kind, i, j, "open")
    return None


def repair(tmask):
    """turn to land (0), in place, every wet cell between two open cells in x or in y, and every wet cell on the edge of the
    array beside an open cell: what is left has no open face the plan refuses, whatever the boxes"""
    o, w = tmask < 0, tmask > 0
    bad = np.zeros_like(w)
    bad[:, 1:-1] |= o[:, :-2] & o[:, 2:]
    bad[1:-1, :] |= o[:-2, :] & o[2:, :]
    bad[:, 0] |= o[:, 1]
    bad[:, -1] |= o[:, -2]
    bad[0, :] |= o[1, :]
    bad[-1, :] |= o[-2, :]
    tmask[w & bad] = 0
    return tmask


def tide(amp, omega, t):
    """amp * sin(omega * t) with the host's sin, as the PSy layers compute ssh_bc"""
    return float(amp) * math.sin(float(omega) * float(t))
