"""CPU tests of the second-order limited tracer transport rule as tests/tracer_muscl_numpy.py
restates it: the two restatements agree bit for bit, wet cells on the array's edge included; what land cells hold, two cells
away included, never reaches a wet cell; a constant nonzero tracer gets the upwind rule's bits; c = 1 stays 1 in the tidal
open channel; a top hat carried by a uniform current is closer to the exact answer than upwind's and stays in its range."""
import numpy as np
import pytest

import open_bc_numpy as B
import tracer_cases as TC
import tracer_muscl_numpy as TM
import tracer_numpy as TN

ULP = 2.0 ** -52


def _both(box, tm, area_t, H, c_in, c_out):
    a = [x.copy() for x in c_out]
    b = [x.copy() for x in c_out]
    flow = [H[n] for n in TC.FLOW]
    TM.tracer_step_muscl(TC.RDT, box, tm, area_t, *flow, c_in, a)
    TM.tracer_step_muscl_scalar(TC.RDT, box, tm, area_t, *flow, c_in, b)
    return a, b


@pytest.mark.parametrize("ld,ny,box,k", [
    (9, 5, (2, 8, 2, 4), 2), (16, 5, (2, 15, 2, 4), 1), (131, 7, (2, 130, 2, 6), 3),      # boxes hugging the ring
    (16, 9, (3, 14, 3, 7), 2), (131, 6, (64, 66, 2, 5), 1),                               # sub-boxes
    (131, 9, (2, 130, 5, 5), 2), (16, 12, (2, 15, 2, 2), 1), (16, 12, (2, 15, 11, 11), 1),  # one row: middle, first, last
    (16, 12, (7, 7, 2, 11), 2), (9, 8, (2, 2, 2, 7), 1), (9, 8, (8, 8, 2, 7), 1),         # one column: middle, first, last
    (16, 6, (9, 8, 2, 5), 1),                                                             # an empty box
])
def test_restatements_agree(ld, ny, box, k):
    """random -1/0/1 masks with wet cells on the array's edge, non-uniform metrics: whole-array numpy == the scalar loop in
    every cell of every output; only wet cells of the box are written"""
    rng = np.random.default_rng(ld * 100 + ny + box[0])
    tm = TC.random_mask(rng, ny, ld)
    edge = np.concatenate([tm[0], tm[-1], tm[:, 0], tm[:, -1]])
    assert (edge > 0).any() and (edge == 0).any()
    area_t, H = TC.flow_inputs(rng, tm)
    c_in, c_out = TC.tracers(rng, tm.shape, k)
    a, b = _both(box, tm, area_t, H, c_in, c_out)
    xs, xe, ys, ye = box
    wet = np.zeros(tm.shape, dtype=bool)
    wet[ys - 1:ye, xs - 1:xe] = tm[ys - 1:ye, xs - 1:xe] > 0
    for n in range(k):
        assert TN.same(a[n], b[n]), (n, np.argwhere(a[n] != b[n])[:5])
        assert (a[n][~wet] == TC.SENTINEL).all()
        assert (a[n][wet] != TC.SENTINEL).all() and np.isfinite(a[n][wet]).all()
    assert wet.any() == (xe >= xs)


def test_the_rule_differs_from_upwind_where_it_should():
    """all wet, away from the edge: the limited value is not the upwind one (the slopes are switched on); in the cells next to
    the array's edge both neighbours' slopes and the cell's own vanish only partly, so nothing is asserted there"""
    rng = np.random.default_rng(3)
    ld, ny = 40, 12
    tm = np.ones((ny, ld), dtype=np.int32)
    area_t, H = TC.flow_inputs(rng, tm)
    c_in, c_out = TC.tracers(rng, tm.shape, 1)
    box = (2, ld - 1, 2, ny - 1)
    up = TC.reference(TC.RDT, box, tm, area_t, H, c_in, c_out)
    a, _ = _both(box, tm, area_t, H, c_in, c_out)
    assert (a[0][3:-3, 3:-3] != up[0][3:-3, 3:-3]).mean() > 0.5


@pytest.mark.parametrize("fill", TC.LAND_FILLS)
def test_land_invariance(fill):
    """six steps; before each, every tracer's land cells are overwritten with `fill` and un / vn with NaN on every face that
    touches land: every wet cell of every step is bit-identical to the run without the overwrites.  The box hugs the ring,
    so the land cells two away from a written cell include cells on the array's edge"""
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
        TM.tracer_step_muscl(TC.RDT, box, tm, area_t, *[H[n] for n in TC.FLOW], clean[0], clean[1])
        H2, c2 = TC.overwrite_land(tm, H, dirty[0], fill)
        TM.tracer_step_muscl(TC.RDT, box, tm, area_t, *[H2[n] for n in TC.FLOW], c2, dirty[1])
        for n in range(k):
            assert TN.same(clean[1][n][wet], dirty[1][n][wet]), (step, n)
            assert np.isfinite(clean[1][n][wet]).all()
        clean = (clean[1], clean[0])
        dirty = (dirty[1], dirty[0])


@pytest.mark.parametrize("value", [1.0, -3.75, 1e-300, 2.5e300])
@pytest.mark.parametrize("ld,ny", [(9, 5), (16, 9), (131, 7)])
def test_a_constant_tracer_gets_the_upwind_bits(ld, ny, value):
    """c = value in every cell: every slope is MC(0, 0) = 0, a face carries c + 0.0 or c - 0.0 = c, and every written cell
    has the bits of tests/tracer_numpy.py's upwind step"""
    rng = np.random.default_rng(ld + ny)
    tm = TC.random_mask(rng, ny, ld)
    area_t, H = TC.flow_inputs(rng, tm)
    c_in = [np.full(tm.shape, value)]
    c_out = [np.full(tm.shape, TC.SENTINEL)]
    box = (2, ld - 1, 2, ny - 1)
    up = TC.reference(TC.RDT, box, tm, area_t, H, c_in, c_out)
    a, b = _both(box, tm, area_t, H, c_in, c_out)
    assert TN.same(a[0], up[0]) and TN.same(b[0], up[0])
    assert (up[0] != TC.SENTINEL).any()


def test_uniform_tracer_stays_uniform_in_the_channel():
    """the tidal open channel of tests/test_tracer_numpy.py, ten steps, c = 1 everywhere: the limited step keeps it 1 within
    that test's bound (steps * 32 ulp)"""
    nx, ny, steps = 96, 24, 10
    tm = TC.channel_user_mask(nx, ny)
    G = TC.uniform_grid(tm, TC.CHANNEL_DXY)
    box = (2, nx + 1, 2, ny + 1)
    assert B.refusal(tm, box, box) is None
    H = TC.channel_state(tm, nx, ny)
    c_in, c_out = TC.channel_tracers(tm)
    rdt = TC.CHANNEL_PRM[0]
    worst_cfl = 0.0
    for step in range(steps):
        TC.cpu_step(G, box, H, B.tide(*TC.CHANNEL_TIDE, (step + 1) * rdt), [], [], TC.CHANNEL_PRM)
        TM.tracer_step_muscl(rdt, box, G.tmask, G.area_t, *[H[k] for k in TC.FLOW], c_in, c_out)
        worst_cfl = max(worst_cfl, TC.cfl(rdt, box, G, H))
        TC.rotate(H)
        c_in, c_out = c_out, c_in
    assert 0.01 < worst_cfl < 0.5, worst_cfl
    err = float(np.abs(c_in[0][tm > 0] - 1.0).max())
    print("constancy: max |c - 1| = %.3g = %.1f ulp after %d steps at CFL %.3g" % (err, err / ULP, steps, worst_cfl))
    assert err <= steps * 32 * ULP, err / ULP
    dye = c_in[1][tm > 0]
    assert np.isfinite(dye).all() and np.ptp(dye) > 0.5


def top_hat(courant=0.25, cells=40, ld=200, ny=5):
    """a 1-D top hat (1 on 40 cells, 0 elsewhere) in a uniform current along x, carried `cells` cells: open west and east
    columns holding 0, land rows south and north, depth 10, area 1, rdt 1, un = courant.  Returns (steps, exact, upwind,
    limited), each a row of wet cells"""
    tm = np.ones((ny, ld), dtype=np.int32)
    tm[0, :] = tm[-1, :] = 0
    tm[1:-1, 0] = tm[1:-1, -1] = -1
    shape = tm.shape
    H = {k: np.zeros(shape) for k in TC.FLOW}
    for k in ("ht", "hu", "hv"):
        H[k][:] = 10.0
    H["un"][1:-1, :-1] = courant
    area_t = np.ones(shape)
    c0 = np.zeros(shape)
    c0[:, 20:60] = 1.0
    steps = int(round(cells / courant))
    assert steps * courant == cells
    exact = np.zeros(shape)
    exact[:, 20 + cells:60 + cells] = 1.0
    box = (2, ld - 1, 2, ny - 1)
    flow = [H[k] for k in TC.FLOW]
    out = []
    for step_fn in (TN.tracer_step, TM.tracer_step_muscl):
        a, b = c0.copy(), c0.copy()
        for _ in range(steps):
            step_fn(1.0, box, tm, area_t, *flow, [a], [b])
            a, b = b, a
        assert TN.same(a[1], a[ny - 2])                               # 1-D: every wet row alike
        out.append(a[2, 1:-1].copy())
    return steps, exact[2, 1:-1], out[0], out[1]


def test_top_hat_beats_upwind_and_stays_in_range():
    """Courant 0.25, 160 steps: the limited scheme's L1 error is strictly below upwind's, and any excursion outside the
    initial range [0, 1] is at most steps * 32 ulp of that range"""
    steps, exact, up, lim = top_hat()
    e_up, e_lim = float(np.abs(up - exact).sum()), float(np.abs(lim - exact).sum())
    mass = float(exact.sum())
    over = max(0.0, float(lim.max()) - 1.0, -float(lim.min()))
    print("top hat: L1 error / mass upwind %.4f, limited %.4f, ratio %.3f; range [%.17g, %.17g], excursion %.3g"
          % (e_up / mass, e_lim / mass, e_lim / e_up, lim.min(), lim.max(), over))
    assert e_lim < e_up
    assert over <= steps * 32 * ULP * 1.0, over / ULP
    assert abs(float(lim.sum()) - mass) <= 1e-9 * mass                # nothing has reached the open east column yet
