"""CPU tests of tests/open_bc_numpy.py, the independent restatement of the open-boundary kernels: the
whole-array numpy form equals the scalar loop bit for bit on odd and even shapes and random {-1, 0, 1} masks that reach every
branch; and the library's plan refuses, through ctypes, exactly the masks open_bc_numpy.refusal names (no device is needed to
refuse a mask, or to accept one without open cells)."""
import ctypes as C

import numpy as np
import pytest

import open_bc_numpy as B

from dl_esm_inf_amd import _cabi

L = _cabi.lib()


def _mask(rng, ny, ld):
    tm = rng.choice(np.array([-1, 0, 1, 1, 1], dtype=np.int32), size=(ny, ld))
    return B.repair(tm)


def _fields(rng, ny, ld):
    h = 1.0 + 20.0 * rng.random((ny, ld))
    h[rng.random((ny, ld)) < 0.05] = 0.0                  # zero depth: c = inf, and nothing may trap
    return h, 0.1 * rng.normal(size=(ny, ld)), 0.1 * rng.normal(size=(ny, ld)), rng.normal(size=(ny, ld))


@pytest.mark.parametrize("ld,ny", [(8, 6), (9, 7), (64, 33), (65, 40), (131, 17)])
def test_numpy_equals_scalar(ld, ny):
    rng = np.random.default_rng(ld * 100 + ny)
    tm = _mask(rng, ny, ld)
    prm = B.params(20.0, 0.00015, 50.0, 9.80665)
    for box in [(2, ld - 1, 2, ny - 1), (3, ld - 2, 2, ny - 3)]:
        assert B.refusal(tm, box, box) is None
        hu, sshn_u, sshn_t, ua = _fields(rng, ny, ld)
        hv, sshn_v, _, va = _fields(rng, ny, ld)
        for fn, sfn, h, s, x in ((B.flather_u, B.flather_u_scalar, hu, sshn_u, ua), (B.flather_v, B.flather_v_scalar, hv, sshn_v, va)):
            a, b = x.copy(), x.copy()
            fn(prm, box, tm, h, s, sshn_t, a)
            sfn(prm, box, tm, h, s, sshn_t, b)
            assert B.same(a, b)
            assert (a != x).any()
        a, b = sshn_t.copy(), sshn_t.copy()
        B.bc_ssh(box, tm, 0.0625, a)
        B.bc_ssh_scalar(box, tm, 0.0625, b)
        assert B.same(a, b) and (a == 0.0625).any()


def test_random_masks_reach_every_branch():
    """west-, east-, south- and north-open faces, faces next to land, and cells the rule skips, all present"""
    rng = np.random.default_rng(7)
    tm = _mask(rng, 40, 64)
    S = lambda a, di, dj: a[1 + dj:39 + dj, 1 + di:63 + di]          # noqa: E731  (box 2..63, 2..39)
    t = S(tm, 0, 0)
    for di, dj in ((1, 0), (0, 1)):
        n = S(tm, di, dj)
        assert ((t < 0) & (n > 0)).any() and ((t > 0) & (n < 0)).any()
        assert ((t < 0) & (n == 0)).any() and ((t < 0) & (n < 0)).any() and ((t > 0) & (n > 0)).any()


def test_flather_sign_and_a_state_at_rest():
    """a west-open face takes ua(iu) - c*(sshn_u(iu) - sshn_t(o)), an east-open one ua(iu) + c*(...); zero stays zero"""
    ld, ny = 8, 3
    tm = np.ones((ny, ld), dtype=np.int32)
    tm[:, 1] = -1
    tm[:, 6] = -1
    prm = B.params(1.0, 0.0, 0.0, 4.0)
    hu = np.ones((ny, ld))
    sshn_u, sshn_t = np.zeros((ny, ld)), np.zeros((ny, ld))
    sshn_t[:, 1], sshn_t[:, 6] = 0.5, 0.25
    ua = np.zeros((ny, ld))
    ua[:, 3] = 1.0
    ua[:, 4] = 3.0
    B.flather_u(prm, (2, 7, 2, 2), tm, hu, sshn_u, sshn_t, ua)
    assert ua[1, 1] == 0.0 - 2.0 * (0.0 - 0.5)                    # face 2: open west, inner face 3
    assert ua[1, 5] == 3.0 + 2.0 * (0.0 - 0.25)                   # face 6: open east, inner face 5
    rest = np.zeros((ny, ld))
    B.flather_u(prm, (2, 7, 2, 2), tm, hu, np.zeros((ny, ld)), np.zeros((ny, ld)), rest)
    assert not rest.any()


def _create(tm, tbox, ubox, vbox):
    ny, ld = tm.shape
    tm = np.ascontiguousarray(tm, dtype=np.int32)
    h = C.c_void_p()
    rc = L.dlesm_obc_create(tm.ctypes.data, ld, ny, C.byref(_cabi.Region(0, 0, *tbox)), C.byref(_cabi.Region(0, 0, *ubox)),
                            C.byref(_cabi.Region(0, 0, *vbox)), C.byref(h))
    if rc == 0:
        L.dlesm_obc_destroy(h)
    return rc


def test_plan_refuses_a_channel_one_cell_wide():
    ld, ny = 12, 8
    tm = np.ones((ny, ld), dtype=np.int32)
    tm[:, 4] = -1
    tm[:, 6] = -1                                                 # column 5: one wet cell between two open ones
    box = (2, ld - 1, 2, ny - 1)
    assert B.refusal(tm, box, box)[3] == "open"
    assert _create(tm, box, box, box) == _cabi.EINVAL
    assert b"open inner face" in L.dlesm_last_error()
    tm = np.ones((ny, ld), dtype=np.int32)
    tm[3, :] = -1
    tm[5, :] = -1                                                 # the same in y
    assert B.refusal(tm, box, box)[0] == "v"
    assert _create(tm, box, box, box) == _cabi.EINVAL


def test_plan_refuses_an_open_face_at_the_edge_of_the_array():
    ld, ny = 10, 6
    tm = np.ones((ny, ld), dtype=np.int32)
    box = (2, ld - 1, 2, ny - 1)
    tm[:, ld - 2], tm[:, ld - 1] = -1, 1                          # face ld-1 open west: inner face ld lies on the edge
    assert B.refusal(tm, (ld - 1, ld - 1, 2, ny - 1), (2, 1, 2, 1)) == ("u", ld - 1, 2, "edge")
    assert _create(tm, box, (ld - 1, ld - 1, 2, ny - 1), (2, 1, 2, 1)) == _cabi.EINVAL
    assert b"edge of the array" in L.dlesm_last_error()
    tm = np.ones((ny, ld), dtype=np.int32)
    tm[ny - 2, :] = -1                                            # v faces (i, ny-1): open south, inner face (i, ny) on the edge
    vb = (2, ld - 1, ny - 1, ny - 1)
    assert B.refusal(tm, (2, 1, 2, 1), vb) == ("v", 2, ny - 1, "edge")
    assert _create(tm, box, (2, 1, 2, 1), vb) == _cabi.EINVAL
    # a box without its one-cell ring is refused like every kernel's
    assert _create(np.ones((ny, ld), dtype=np.int32), box, (1, ld - 1, 2, ny - 1), box) == _cabi.EINVAL


def test_plan_accepts_a_mask_without_open_cells_and_empty_boxes():
    """nothing to upload: accepted without touching a device, every list empty"""
    ld, ny = 16, 9
    tm = np.ones((ny, ld), dtype=np.int32)
    tm[:, :3] = 0
    box = (2, ld - 1, 2, ny - 1)
    for tb, ub, vb in ((box, box, box), ((2, 1, 2, 1), (5, 4, 2, 8), box)):
        h = C.c_void_p()
        assert L.dlesm_obc_create(tm.ctypes.data, ld, ny, C.byref(_cabi.Region(0, 0, *tb)), C.byref(_cabi.Region(0, 0, *ub)),
                                  C.byref(_cabi.Region(0, 0, *vb)), C.byref(h)) == 0
        n = [C.c_int(-1) for _ in range(3)]
        assert L.dlesm_obc_counts(h, *[C.byref(x) for x in n]) == 0
        assert [x.value for x in n] == [0, 0, 0]
        assert L.dlesm_obc_destroy(h) == 0


@pytest.mark.parametrize("seed", range(6))
def test_plan_refuses_exactly_what_the_restatement_names(seed):
    """random unrepaired masks: EINVAL exactly when open_bc_numpy.refusal names a face (an accepted plan needs a device to
    hold its lists: without one the library says so)"""
    rng = np.random.default_rng(seed)
    ld, ny = 14 + seed, 9
    tm = rng.choice(np.array([-1, 0, 1, 1, 1, 1, 1, 1], dtype=np.int32), size=(ny, ld))
    if seed % 2:
        tm = B.repair(tm)
    box = (2, ld - 1, 2, ny - 1)
    rc = _create(tm, box, box, box)
    if B.refusal(tm, box, box) is None:
        assert rc in (0, _cabi.ENODEV), rc
    else:
        assert rc == _cabi.EINVAL
