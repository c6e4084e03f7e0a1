"""CPU tests of the momentum / next_ssh checker (tests/momentum_numpy.py): its whole-array numpy form equals its scalar
loop bit for bit, on odd and even shapes, with masks that take every branch of DESIGN.md section 6.5, and a state at rest
stays at rest."""
import numpy as np
import pytest

import momentum_numpy as M

SHAPES = [(9, 11), (10, 12), (17, 40), (6, 7)]            # (ny, ld)
PRM = M.params(rdt=20.0, cbfr=0.00015, visc=50.0, g=9.80665)


def _grid(rng, ny, ld):
    """random -1/0/1 mask with a coastline (a land block), non-uniform metrics, Coriolis from a non-constant latitude"""
    tm = rng.integers(-1, 2, (ny, ld)).astype(np.int32)
    tm[: ny // 3, : ld // 3] = 0
    tm[-2:, -3:] = 1
    G = {}
    for k in M.GRID_ARRAYS[1:9]:
        G[k] = 900.0 + 200.0 * rng.random((ny, ld))
    G["area_u"] = G["area_u"] * 1000.0
    G["area_v"] = G["area_v"] * 1000.0
    G["fcor_u"] = M.coriolis(40.0 + 20.0 * rng.random((ny, ld)), 7.292116e-5, np.pi / 180.0)
    G["fcor_v"] = M.coriolis(40.0 + 20.0 * rng.random((ny, ld)), 7.292116e-5, np.pi / 180.0)
    return M.SimpleNamespace(tmask=tm, **G)


def _fields(rng, ny, ld):
    """un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, ssha_v: velocities of both signs with +-0.0 among them"""
    def vel():
        v = rng.normal(0.0, 0.3, (ny, ld))
        pick = rng.random((ny, ld))
        v[pick < 0.15] = 0.0
        v[(pick >= 0.15) & (pick < 0.3)] = -0.0
        return v
    un, vn = vel(), vel()
    depth = [10.0 + rng.random((ny, ld)) for _ in range(3)]
    ssh = [0.1 * rng.normal(size=(ny, ld)) for _ in range(5)]
    ht, hu, hv = depth
    sshn_t, sshn_u, sshn_v, ssha_u, ssha_v = ssh
    return un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, ssha_v


def _boxes(ny, ld):
    return [(2, ld - 1, 2, ny - 1), (3, ld - 2, 2, ny - 2), (2, 2, 2, 2)]


@pytest.mark.parametrize("ny,ld", SHAPES)
def test_vectorised_equals_scalar_loop(ny, ld):
    rng = np.random.default_rng(ny * 100 + ld)
    G = _grid(rng, ny, ld)
    un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, ssha_v = _fields(rng, ny, ld)
    ins = (un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v)
    seen = set()
    for box in _boxes(ny, ld):
        a, b = np.full((ny, ld), -7.0), np.full((ny, ld), -7.0)
        M.momentum_u(PRM, G, box, *ins, ssha_u, a)
        M.momentum_u_scalar(PRM, G, box, *ins, ssha_u, b)
        assert M.same(a, b), ("u", box)
        seen.add(("u", bool((a != -7.0).any())))
        a, b = np.full((ny, ld), -7.0), np.full((ny, ld), -7.0)
        M.momentum_v(PRM, G, box, *ins, ssha_v, a)
        M.momentum_v_scalar(PRM, G, box, *ins, ssha_v, b)
        assert M.same(a, b), ("v", box)
        for area, di, dj, vec, sca in ((G.area_u, 1, 0, M.next_sshu, M.next_sshu_scalar),
                                       (G.area_v, 0, 1, M.next_sshv, M.next_sshv_scalar)):
            a, b = np.full((ny, ld), -7.0), np.full((ny, ld), -7.0)
            vec(box, G.tmask, G.dx_t, area, sshn_t, a)
            sca(box, G.tmask, G.dx_t, area, sshn_t, b)
            assert M.same(a, b), ("next_ssh", di, dj, box)
    # the fused form is the two loop nests over their own boxes
    ub, vb = (2, ld - 1, 2, ny - 2), (3, ld - 1, 2, ny - 1)
    ua, va, ua2, va2 = (np.full((ny, ld), 5.0) for _ in range(4))
    M.momentum(PRM, G, ub, vb, *ins, ssha_u, ssha_v, ua, va)
    M.momentum_u_scalar(PRM, G, ub, *ins, ssha_u, ua2)
    M.momentum_v_scalar(PRM, G, vb, *ins, ssha_v, va2)
    assert M.same(ua, ua2) and M.same(va, va2)


@pytest.mark.parametrize("ny,ld", [(17, 40)])
def test_every_branch_is_taken(ny, ld):
    """the random cases above reach every branch of s(), sw/nw/ww/ew and next_ssh: counted on the scalar restatement's
    own operands"""
    rng = np.random.default_rng(ny * 100 + ld)
    G = _grid(rng, ny, ld)
    un, vn = _fields(rng, ny, ld)[:2]
    T = G.tmask
    box = (2, ld - 1, 2, ny - 1)
    xs, xe, ys, ye = box
    wet_u = [(i, j) for j in range(ys, ye + 1) for i in range(xs, xe + 1) if T[j - 1, i - 1] > 0 and T[j - 1, i] > 0]
    wet_v = [(i, j) for j in range(ys, ye + 1) for i in range(xs, xe + 1) if T[j - 1, i - 1] > 0 and T[j, i - 1] > 0]
    assert wet_u and wet_v
    sw = {bool(T[j - 2, i - 1] > 0 and T[j - 2, i] > 0) for i, j in wet_u}
    nw = {bool(T[j, i - 1] > 0 and T[j, i] > 0) for i, j in wet_u}
    ww = {bool(T[j - 1, i - 2] > 0 and T[j, i - 2] > 0) for i, j in wet_v}
    ew = {bool(T[j - 1, i] > 0 and T[j, i] > 0) for i, j in wet_v}
    assert sw == nw == ww == ew == {True, False}
    signs = {(float(np.copysign(1.0, un[j - 1, i - 1])), un[j - 1, i - 1] == 0.0) for i, j in wet_u}
    assert {(1.0, True), (-1.0, True), (1.0, False), (-1.0, False)} <= signs
    pairs = {(int(np.sign(T[j - 1, i - 1])), int(np.sign(T[j - 1, i]))) for j in range(ys, ye + 1) for i in range(xs, xe + 1)}
    assert {(1, 1), (1, 0), (0, 1), (-1, 1), (1, -1), (0, 0), (-1, -1)} <= pairs


@pytest.mark.parametrize("ny,ld", SHAPES)
def test_state_at_rest_stays_at_rest(ny, ld):
    """un = vn = 0 and a flat sea surface: ua == va == 0 on every written cell (every term carries a velocity or a
    surface difference), nothing else written"""
    rng = np.random.default_rng(ny + ld)
    G = _grid(rng, ny, ld)
    _, _, ht, _, hu, _, hv, _, _, _ = _fields(rng, ny, ld)
    zero = np.zeros((ny, ld))
    flat = np.full((ny, ld), 0.25)
    box = (2, ld - 1, 2, ny - 1)
    ua, va = np.full((ny, ld), np.nan), np.full((ny, ld), np.nan)
    M.momentum(PRM, G, box, box, zero, zero, ht, flat, hu, flat, hv, flat, flat, flat, ua, va)
    for out, di, dj in ((ua, 1, 0), (va, 0, 1)):
        written = ~np.isnan(out)
        assert written.any()
        assert np.all(out[written] == 0.0)
        xs, xe, ys, ye = box
        T = G.tmask
        want = np.zeros((ny, ld), dtype=bool)
        want[ys - 1:ye, xs - 1:xe] = (T[ys - 1:ye, xs - 1:xe] > 0) & (T[ys - 1 + dj:ye + dj, xs - 1 + di:xe + di] > 0)
        assert np.array_equal(written, want)
