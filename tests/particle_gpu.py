"""What the GPU tests of the three particle steps share (test_gpu_drifter.py, test_gpu_dispersal.py, test_gpu_random_walk.py,
test_gpu_particle_step_refusals.py): the device fixture, the case's arrays on the device -- made once a module --, the
comparison with a reference, and the refusals every step shares.  A plain module like drifter_cases.py; nothing runs on import."""
import ctypes as C

import numpy as np
import pytest

import dispersal_cases as PC
import drifter_cases as DC
import drifter_numpy as DN

SENT = DC.SENTINEL
SLACK = 64
NS = [1, 63, 64, 65, 257, 1000, 70001]
_DEV = {}


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    import dl_esm_inf_amd as d
    torch.cuda.set_device(0)
    d.parallel_init(0, 1)
    yield torch, d, d._cabi.lib()
    _DEV.clear()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _up(torch, a, off=0):
    """a host array on the device, its base `off` elements behind an allocation's"""
    flat = torch.empty(a.size + off, dtype=torch.from_numpy(a).dtype, device="cuda")
    t = flat[off:].view(a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def _flow(torch, ld, off):
    """(tm, dx_t, dy_t, un, vn) on the device with leading dimension ld, bases offset by `off` elements; made once"""
    key = (ld, off)
    if key not in _DEV:
        tm, dx_t, dy_t, un, vn = DC.flow()
        _DEV[key] = [_up(torch, DC.embed(tm, ld, 0), off)] + [_up(torch, DC.embed(a, ld, np.nan), off)
                                                              for a in (dx_t, dy_t, un, vn)]
    return _DEV[key]


def _ids(torch, off=0):
    """the pool's identities on the device; made once"""
    key = ("ids", off)
    if key not in _DEV:
        _DEV[key] = _up(torch, PC.ids(), off)
    return _DEV[key]


def _particles(torch, n, off=0, pool=None):
    """the first n of the pool, in arrays with SLACK sentinel elements behind them"""
    px, py, st = pool or DC.particles()
    out = []
    for a, fill in ((px, SENT), (py, SENT), (st, -9)):
        h = np.full(n + SLACK, fill, dtype=a.dtype)
        h[:n] = a[:n]
        out.append(_up(torch, h, off))
    return out


def _check(P, n, want, what):
    got = [t.cpu().numpy() for t in P]
    assert DN.same(got[0][:n], want[0][:n]), (what, "px")
    assert DN.same(got[1][:n], want[1][:n]), (what, "py")
    assert (got[2][:n] == want[2][:n]).all(), (what, "status")
    assert (got[0][n:] == SENT).all() and (got[1][n:] == SENT).all() and (got[2][n:] == -9).all(), (what, "slack")
    return got


def _equal(torch, A, B):
    return all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(A, B))


def shared_refusals(raw, EINVAL, max_sub, Fp, Pp, n):
    """everything dlesm_drifter_step_f64 refuses, asked of the entry behind raw(Fp, Pp, n_=, nsub=, h=, b=, ny=, ld_=): Fp and
    Pp are the addresses of the five inputs and of px, py, status (None: a null pointer), on the 26 x 22 case"""
    for k in range(5):                                                              # a null input
        assert raw(Fp[:k] + [None] + Fp[k + 1:], Pp) == EINVAL, k
    for k in range(3):                                                              # a null particle array
        assert raw(Fp, Pp[:k] + [None] + Pp[k + 1:]) == EINVAL, k
    for k in range(1, 5):                                                           # a double array not 8-byte aligned
        G = list(Fp)
        G[k] += 4
        assert raw(G, Pp) == EINVAL, k
    assert raw([Fp[0] + 2] + Fp[1:], Pp) == EINVAL                                  # the mask not 4-byte aligned
    assert raw(Fp, [Pp[0] + 4, Pp[1], Pp[2]]) == EINVAL and raw(Fp, [Pp[0], Pp[1] + 4, Pp[2]]) == EINVAL
    assert raw(Fp, [Pp[0], Pp[1], Pp[2] + 2]) == EINVAL
    assert raw(Fp, Pp, n_=-1) == EINVAL
    assert raw(Fp, Pp, nsub=0) == EINVAL and raw(Fp, Pp, nsub=max_sub + 1) == EINVAL
    for h in (float("nan"), float("inf"), float("-inf")):
        assert raw(Fp, Pp, h=h) == EINVAL
    for b in ((1, 25, 2, 21), (2, 26, 2, 21), (2, 25, 1, 21), (2, 25, 2, 22)):      # no room for the ring
        assert raw(Fp, Pp, b=b) == EINVAL, b
    assert raw(Fp, Pp, ld_=0) == EINVAL and raw(Fp, Pp, ny=0) == EINVAL
    assert raw(Fp, [Pp[0], Pp[0], Pp[2]]) == EINVAL and raw(Fp, [Pp[0], Pp[1], Pp[0]]) == EINVAL       # particle arrays overlap
    assert raw(Fp, [Pp[0], Pp[0] + 8 * (n - 1), Pp[2]]) == EINVAL
    for k in range(5):                                                              # ... or lie in an input
        assert raw(Fp, [Fp[k], Pp[1], Pp[2]]) == EINVAL and raw(Fp, [Pp[0], Pp[1], Fp[k]]) == EINVAL, k
