"""CPU tests of the tracer transport rule as tests/tracer_numpy.py restates it: the two
restatements agree bit for bit; what land cells and faces that touch land hold never reaches a wet cell; a uniform tracer
stays uniform and a tracer in [0, 1] stays there in a tidal open channel driven by the existing restatements of the
NEMOLite2D-class step."""
import numpy as np
import pytest

import open_bc_numpy as B
import tracer_cases as TC
import tracer_numpy as TN

ULP = 2.0 ** -52


@pytest.mark.parametrize("ld,ny,box,k", [(37, 23, (2, 36, 2, 22), 3), (64, 20, (5, 60, 3, 18), 1), (6, 5, (2, 5, 2, 4), 2),
                                         (40, 12, (7, 7, 2, 11), 2), (40, 12, (9, 8, 2, 11), 1)])
def test_restatements_agree(ld, ny, box, k):
    """random -1/0/1 masks, non-uniform metrics: whole-array numpy == the scalar loop, in every cell of every output"""
    rng = np.random.default_rng(ld * 100 + ny)
    tm = TC.random_mask(rng, ny, ld)
    area_t, H = TC.flow_inputs(rng, tm)
    c_in, c_out = TC.tracers(rng, tm.shape, k)
    a = TC.reference(TC.RDT, box, tm, area_t, H, c_in, c_out)
    b = [x.copy() for x in c_out]
    TN.tracer_step_scalar(TC.RDT, box, tm, area_t, *[H[n] for n in TC.FLOW], c_in, b)
    xs, xe, ys, ye = box
    wet = np.zeros(tm.shape, dtype=bool)
    wet[ys - 1:ye, xs - 1:xe] = tm[ys - 1:ye, xs - 1:xe] > 0
    for n in range(k):
        assert TN.same(a[n], b[n]), n
        assert (a[n][~wet] == TC.SENTINEL).all()                  # land, open cells and everything outside the box
        assert (a[n][wet] != TC.SENTINEL).all() and np.isfinite(a[n][wet]).all()
    assert wet.any() == (xe >= xs)


@pytest.mark.parametrize("fill", TC.LAND_FILLS)
def test_land_invariance(fill):
    """six steps; before each, every tracer's land cells are overwritten with `fill` and un / vn with NaN on every face that
    touches land: every wet cell of every step is bit-identical to the run without the overwrites"""
    ld, ny, k = 61, 33, 2
    box = (2, ld - 1, 2, ny - 1)
    rng = np.random.default_rng(7)
    tm = TC.random_mask(rng, ny, ld)
    area_t, H = TC.flow_inputs(rng, tm)
    c0, _ = TC.tracers(rng, tm.shape, k)
    clean = ([c.copy() for c in c0], [c.copy() for c in c0])
    dirty = ([c.copy() for c in c0], [c.copy() for c in c0])
    wet = tm > 0
    assert (tm == 0).sum() > 100 and (tm < 0).sum() > 100
    for step in range(6):
        TN.tracer_step(TC.RDT, box, tm, area_t, *[H[n] for n in TC.FLOW], clean[0], clean[1])
        H2, c2 = TC.overwrite_land(tm, H, dirty[0], fill)
        assert np.isnan(H2["un"]).sum() > 100 and np.isnan(H2["vn"]).sum() > 100
        TN.tracer_step(TC.RDT, box, tm, area_t, *[H2[n] for n in TC.FLOW], c2, dirty[1])
        for n in range(k):
            assert TN.same(clean[1][n][wet], dirty[1][n][wet]), (step, n)
            assert np.isfinite(clean[1][n][wet]).all()
        clean = (clean[1], clean[0])
        dirty = (dirty[1], dirty[0])


def _channel_loop(steps):
    nx, ny = 96, 24
    tm = TC.channel_user_mask(nx, ny)
    G = TC.uniform_grid(tm, TC.CHANNEL_DXY)
    box = (2, nx + 1, 2, ny + 1)
    assert B.refusal(tm, box, box) is None
    H = TC.channel_state(tm, nx, ny)
    c_in, c_out = TC.channel_tracers(tm)
    rdt = TC.CHANNEL_PRM[0]
    worst_cfl = 0.0
    for step in range(steps):
        TC.cpu_step(G, box, H, B.tide(*TC.CHANNEL_TIDE, (step + 1) * rdt), c_in, c_out, TC.CHANNEL_PRM)
        worst_cfl = max(worst_cfl, TC.cfl(rdt, box, G, H))
        TC.rotate(H)
        c_in, c_out = c_out, c_in
    return tm, H, c_in, worst_cfl


@pytest.fixture(scope="module")
def channel():
    return _channel_loop(10)


def test_uniform_tracer_stays_uniform(channel):
    """a tidal open channel, ten steps, c = 1 everywhere (the open cells included): with continuity's own r1..r4 and the ssha
    of the same step the tracer stays 1 up to rounding -- about eight roundings a step, each amplified by at most
    1 + 4 CFL, so 32 ulp a step is a safe cap"""
    tm, H, c, worst_cfl = channel
    assert worst_cfl < 0.5, worst_cfl                             # the precondition of the bound, and of monotonicity
    assert worst_cfl > 0.01 and float(np.abs(H["vn"]).max()) > 0.01      # the water moves, and not along x alone
    err = float(np.abs(c[0][tm > 0] - 1.0).max())
    print("constancy: max |c - 1| = %.3g = %.1f ulp after 10 steps at CFL %.3g" % (err, err / ULP, worst_cfl))
    assert err <= 10 * 32 * ULP, err / ULP


def test_tracer_stays_in_range(channel):
    """the same loop, a tracer in [0, 1]: first-order upwind is monotone under CFL < 0.5, so it stays in [0, 1] up to the
    same rounding allowance"""
    tm, H, c, worst_cfl = channel
    assert worst_cfl < 0.5, worst_cfl
    tol = 10 * 32 * ULP
    wet = c[1][tm > 0]
    print("range: min %.17g, max %.17g" % (wet.min(), wet.max()))
    assert wet.min() >= 0.0 - tol and wet.max() <= 1.0 + tol
    assert wet.max() - wet.min() > 0.5                            # it is no constant
