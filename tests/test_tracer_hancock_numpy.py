"""CPU tests of the time-centred limited tracer transport rule as tests/tracer_hancock_numpy.py
restates it: the two restatements agree bit for bit at an rdt that puts faces on both sides of a Courant number of 1; what
land cells hold -- in the tracers, in un / vn and in area_t, ht, sshn_t -- never reaches a wet cell; a constant nonzero tracer
gets the upwind rule's bits; c = 1 stays 1 in the tidal open channel; a Gaussian carried by a uniform current is closer to
the exact answer than section 6.11's and upwind's, a top hat closer than upwind's, in one and in two dimensions, and all
stay in their range."""
import numpy as np
import pytest

import open_bc_numpy as B
import tracer_cases as TC
import tracer_hancock_numpy as TH
import tracer_muscl_numpy as TM
import tracer_numpy as TN

ULP = 2.0 ** -52
RDT_BIG = 3.0e6         # TC.RDT = 600 leaves every Courant number of the shared inputs below 7e-4: n >= 1 would never run

SHAPES = [
    (9, 5, (2, 8, 2, 4), 2), (16, 5, (2, 15, 2, 4), 1), (131, 7, (2, 130, 2, 6), 3),      # boxes hugging the ring
    (16, 9, (3, 14, 3, 7), 2), (131, 6, (64, 66, 2, 5), 1),                               # sub-boxes
    (131, 9, (2, 130, 5, 5), 2), (16, 12, (2, 15, 2, 2), 1), (16, 12, (2, 15, 11, 11), 1),  # one row: middle, first, last
    (16, 12, (7, 7, 2, 11), 2), (9, 8, (2, 2, 2, 7), 1), (9, 8, (8, 8, 2, 7), 1),         # one column: middle, first, last
    (16, 6, (9, 8, 2, 5), 1),                                                             # an empty box
]


def _case(ld, ny, box, k):
    rng = np.random.default_rng(ld * 100 + ny + box[0])
    tm = TC.random_mask(rng, ny, ld)
    area_t, H = TC.flow_inputs(rng, tm)
    c_in, c_out = TC.tracers(rng, tm.shape, k)
    return tm, area_t, H, c_in, c_out


def _both(rdt, box, tm, area_t, H, c_in, c_out):
    a = [x.copy() for x in c_out]
    b = [x.copy() for x in c_out]
    flow = [H[n] for n in TC.FLOW]
    TH.tracer_step_hancock(rdt, box, tm, area_t, *flow, c_in, a)
    TH.tracer_step_hancock_scalar(rdt, box, tm, area_t, *flow, c_in, b)
    return a, b


@pytest.mark.parametrize("rdt", [RDT_BIG, TC.RDT])
@pytest.mark.parametrize("ld,ny,box,k", SHAPES)
def test_restatements_agree(ld, ny, box, k, rdt):
    """random -1/0/1 masks with wet cells on the array's edge, non-uniform metrics: whole-array numpy == the scalar loop in
    every cell of every output; only wet cells of the box are written"""
    tm, area_t, H, c_in, c_out = _case(ld, ny, box, k)
    edge = np.concatenate([tm[0], tm[-1], tm[:, 0], tm[:, -1]])
    assert (edge > 0).any() and (edge == 0).any()
    a, b = _both(rdt, box, tm, area_t, H, c_in, c_out)
    xs, xe, ys, ye = box
    wet = np.zeros(tm.shape, dtype=bool)
    wet[ys - 1:ye, xs - 1:xe] = tm[ys - 1:ye, xs - 1:xe] > 0
    for n in range(k):
        assert TN.same(a[n], b[n]), (n, np.argwhere(a[n] != b[n])[:5])
        assert (a[n][~wet] == TC.SENTINEL).all()
        assert (a[n][wet] != TC.SENTINEL).all() and np.isfinite(a[n][wet]).all()
    assert wet.any() == (xe >= xs)


def test_the_big_rdt_runs_both_branches_of_the_factor():
    """over the faces of the wet cells of every box above taken together, and on each array of the GPU tests' matrix with
    its seed, at least a tenth have 0 < n < 1 and at least a tenth n >= 1; at TC.RDT none reaches 1"""
    mid = big = total = 0.0
    for ld, ny, box, k in SHAPES:
        if box[1] < box[0]:
            continue
        tm, area_t, H, _, _ = _case(ld, ny, box, k)
        faces = 4 * int((tm[box[2] - 1:box[3], box[0] - 1:box[1]] > 0).sum())
        m, b = TH.face_shares(RDT_BIG, box, tm, area_t, *[H[n] for n in TC.FLOW])
        mid, big, total = mid + m * faces, big + b * faces, total + faces
        assert TH.face_shares(TC.RDT, box, tm, area_t, *[H[n] for n in TC.FLOW])[1] == 0.0
    print("shares over %d faces: 0 < n < 1 %.3f, n >= 1 %.3f" % (total, mid / total, big / total))
    assert mid / total >= 0.10 and big / total >= 0.10
    sub = {(1300, 8): (301, 1291, 3, 6)}                  # the GPU tests sweep this array on a sub-box only
    for ld, ny in ((260, 9), (131, 7), (130, 6), (64, 5), (1000, 9), (1300, 8), (4100, 7), (12, 4200), (13, 4200), (66, 4200)):
        rng = np.random.default_rng(ld * 7 + ny)
        tm = TC.random_mask(rng, ny, ld)
        area_t, H = TC.flow_inputs(rng, tm)
        m, b = TH.face_shares(RDT_BIG, sub.get((ld, ny), (2, ld - 1, 2, ny - 1)), tm, area_t, *[H[n] for n in TC.FLOW])
        print("%dx%d: 0 < n < 1 %.3f, n >= 1 %.3f" % (ld, ny, m, b))
        assert m >= 0.10 and b >= 0.10


def test_the_rule_differs_from_muscl_where_it_should():
    """all wet, away from the edge, Courant numbers below 1: the factor is not 0.5, so the value is not section 6.11's"""
    rng = np.random.default_rng(3)
    ld, ny = 40, 12
    tm = np.ones((ny, ld), dtype=np.int32)
    area_t, H = TC.flow_inputs(rng, tm)
    c_in, c_out = TC.tracers(rng, tm.shape, 1)
    box = (2, ld - 1, 2, ny - 1)
    lim = [x.copy() for x in c_out]
    TM.tracer_step_muscl(RDT_BIG / 8, box, tm, area_t, *[H[n] for n in TC.FLOW], c_in, lim)
    a, _ = _both(RDT_BIG / 8, box, tm, area_t, H, c_in, c_out)
    assert (a[0][3:-3, 3:-3] != lim[0][3:-3, 3:-3]).mean() > 0.5


def overwrite_land(tm, area_t, H, c_in, fill):
    """TC.overwrite_land, and NaN in area_t, ht and sshn_t on land as well"""
    H2, c2 = TC.overwrite_land(tm, H, c_in, fill)
    a2 = area_t.copy()
    for x in (a2, H2["ht"], H2["sshn_t"]):
        x[tm == 0] = np.nan
    return a2, H2, c2


@pytest.mark.parametrize("rdt", [RDT_BIG, TC.RDT])
@pytest.mark.parametrize("fill", TC.LAND_FILLS)
def test_land_invariance(fill, rdt):
    """six steps; before each, every tracer's land cells are overwritten with `fill`, un / vn with NaN on every face that
    touches land, and area_t, ht, sshn_t with NaN on land: every wet cell of every step is bit-identical to the run without
    the overwrites.  (At the big rdt the tracers grow without bound -- the Courant numbers pass 1 -- but stay finite for
    six steps: the comparison is of bits, not of physics.)"""
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
        TH.tracer_step_hancock(rdt, box, tm, area_t, *[H[n] for n in TC.FLOW], clean[0], clean[1])
        a2, H2, c2 = overwrite_land(tm, area_t, H, dirty[0], fill)
        assert np.isnan(a2).any() and np.isnan(H2["ht"]).any() and np.isnan(H2["sshn_t"]).any()
        TH.tracer_step_hancock(rdt, box, tm, a2, *[H2[n] for n in TC.FLOW], c2, dirty[1])
        for n in range(k):
            assert TN.same(clean[1][n][wet], dirty[1][n][wet]), (step, n)
            assert np.isfinite(clean[1][n][wet]).all()
        clean = (clean[1], clean[0])
        dirty = (dirty[1], dirty[0])


@pytest.mark.parametrize("rdt", [RDT_BIG, TC.RDT])
@pytest.mark.parametrize("value", [1.0, -3.75, 1e-300, 2.5e300])
@pytest.mark.parametrize("ld,ny", [(9, 5), (16, 9), (131, 7)])
def test_a_constant_tracer_gets_the_upwind_bits(ld, ny, value, rdt):
    """c = value in every cell: every slope is MC(0, 0) = 0, a face carries c + g*0.0 or c - g*0.0 = c with g finite, and
    every written cell has the bits of tests/tracer_numpy.py's upwind step"""
    rng = np.random.default_rng(ld + ny)
    tm = TC.random_mask(rng, ny, ld)
    area_t, H = TC.flow_inputs(rng, tm)
    c_in = [np.full(tm.shape, value)]
    c_out = [np.full(tm.shape, TC.SENTINEL)]
    box = (2, ld - 1, 2, ny - 1)
    up = TC.reference(rdt, box, tm, area_t, H, c_in, c_out)
    a, b = _both(rdt, box, tm, area_t, H, c_in, c_out)
    assert TN.same(a[0], up[0]) and TN.same(b[0], up[0])
    assert (up[0] != TC.SENTINEL).any()


def test_uniform_tracer_stays_uniform_in_the_channel():
    """the tidal open channel of tests/test_tracer_numpy.py, ten steps, c = 1 everywhere: the step keeps it 1 within that
    test's bound (steps * 32 ulp)"""
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
        TH.tracer_step_hancock(rdt, box, G.tmask, G.area_t, *[H[k] for k in TC.FLOW], c_in, c_out)
        worst_cfl = max(worst_cfl, TC.cfl(rdt, box, G, H))
        TC.rotate(H)
        c_in, c_out = c_out, c_in
    assert 0.01 < worst_cfl < 0.5, worst_cfl
    err = float(np.abs(c_in[0][tm > 0] - 1.0).max())
    print("constancy: max |c - 1| = %.3g = %.1f ulp after %d steps at CFL %.3g" % (err, err / ULP, steps, worst_cfl))
    assert err <= steps * 32 * ULP, err / ULP
    dye = c_in[1][tm > 0]
    assert np.isfinite(dye).all() and np.ptp(dye) > 0.5


# ---- carried profiles ---------------------------------------------------------------------------------------------------
SCHEMES = (TN.tracer_step, TM.tracer_step_muscl, TH.tracer_step_hancock)


def carry_1d(profile, courant, cells=40, ld=200, ny=5):
    """test_tracer_muscl_numpy.top_hat's channel -- a uniform current along x, open west and east columns, land rows south
    and north, depth 10, area 1, rdt 1, un = courant -- carrying `profile` (a function of the 0-based column) `cells` cells.
    Returns (steps, initial, exact, [upwind, limited, hancock]), each a row of wet cells"""
    tm = np.ones((ny, ld), dtype=np.int32)
    tm[0, :] = tm[-1, :] = 0
    tm[1:-1, 0] = tm[1:-1, -1] = -1
    shape = tm.shape
    H = {k: np.zeros(shape) for k in TC.FLOW}
    for k in ("ht", "hu", "hv"):
        H[k][:] = 10.0
    H["un"][1:-1, :-1] = courant
    area_t = np.ones(shape)
    x = np.arange(ld, dtype=np.float64)
    c0 = np.tile(profile(x), (ny, 1))
    exact = np.tile(profile(x - cells), (ny, 1))
    steps = int(round(cells / courant))
    assert steps * courant == cells
    box = (2, ld - 1, 2, ny - 1)
    flow = [H[k] for k in TC.FLOW]
    out = []
    for step_fn in SCHEMES:
        a, b = c0.copy(), c0.copy()
        for _ in range(steps):
            step_fn(1.0, box, tm, area_t, *flow, [a], [b])
            a, b = b, a
        assert TN.same(a[1], a[ny - 2])                               # 1-D: every wet row alike
        out.append(a[2, 1:-1].copy())
    return steps, c0[2, 1:-1], exact[2, 1:-1], out


def gaussian(x):
    return np.exp(-((x - 40.0) / 8.0) ** 2)


def hat(x):
    return np.where((x >= 20) & (x < 60), 1.0, 0.0)


def _report(name, steps, c0, exact, runs):
    mass = float(exact.sum())
    l1 = [float(np.abs(r - exact).sum()) / mass for r in runs]
    lo, hi = float(c0.min()), float(c0.max())
    over = [max(0.0, float(r.max()) - hi, lo - float(r.min())) for r in runs]
    print("%s: L1 error / mass upwind %.4f, limited %.4f, hancock %.4f; hancock's excursion from [%.3g, %.3g] %.3g (%d steps)"
          % (name, l1[0], l1[1], l1[2], lo, hi, over[2], steps))
    return l1, over, mass, (hi - lo)


@pytest.mark.parametrize("courant", [0.25, 0.5])
def test_gaussian_beats_limited_and_upwind(courant):
    """exp(-((x - 40) / 8)^2) carried 40 cells: L1 strictly below section 6.11's and upwind's; any excursion from the initial
    range at most steps * 32 ulp of that range.  (The issue's table: 0.3179 / 0.1886 / 0.0182 at 0.25, 0.2345 / 0.3317 /
    0.0118 at 0.5)"""
    steps, c0, exact, runs = carry_1d(gaussian, courant)
    l1, over, _, span = _report("gaussian at %g" % courant, steps, c0, exact, runs)
    assert l1[2] < l1[1] and l1[2] < l1[0]
    assert over[2] <= steps * 32 * ULP * span, over[2] / ULP


def test_top_hat_beats_upwind_and_keeps_its_mass():
    """Courant 0.25, 160 steps: L1 strictly below upwind's (section 6.11's compressive form is sharper on a discontinuity:
    nothing is asked against it), the range [0, 1] kept within steps * 32 ulp, the mass within 1e-9.  (The issue's table:
    0.2180 / 0.0251 / 0.0639)"""
    steps, c0, exact, runs = carry_1d(hat, 0.25)
    l1, over, mass, span = _report("top hat at 0.25", steps, c0, exact, runs)
    assert l1[2] < l1[0]
    assert over[2] <= steps * 32 * ULP * span, over[2] / ULP
    assert abs(float(runs[2].sum()) - mass) <= 1e-9 * mass            # nothing has reached the open east column yet


def carry_2d(cu, cv, n=96, steps=96, width=6.0):
    """a 96 x 96 array: an outer frame of land, a ring of open cells inside it, uniform un and vn on every face between two
    cells that are not land, depth 10, area 1, rdt 1; a Gaussian blob of the given width carried `steps` steps.  Returns
    (initial, exact, [upwind, limited, hancock]) on the wet cells"""
    tm = np.ones((n, n), dtype=np.int32)
    tm[1, :] = tm[-2, :] = tm[:, 1] = tm[:, -2] = -1
    tm[0, :] = tm[-1, :] = tm[:, 0] = tm[:, -1] = 0
    shape = tm.shape
    H = {k: np.zeros(shape) for k in TC.FLOW}
    for k in ("ht", "hu", "hv"):
        H[k][:] = 10.0
    H["un"][1:-1, 1:-2] = cu
    H["vn"][1:-2, 1:-1] = cv
    area_t = np.ones(shape)
    jj, ii = np.mgrid[0:n, 0:n].astype(np.float64)
    x0, y0 = 30.0, 30.0

    def blob(dx, dy):
        return np.exp(-(((ii - x0 - dx) / width) ** 2 + ((jj - y0 - dy) / width) ** 2))
    c0, exact = blob(0.0, 0.0), blob(cu * steps, cv * steps)
    box = (2, n - 1, 2, n - 1)
    flow = [H[k] for k in TC.FLOW]
    wet = tm > 0
    out = []
    for step_fn in SCHEMES:
        a, b = c0.copy(), c0.copy()
        for _ in range(steps):
            step_fn(1.0, box, tm, area_t, *flow, [a], [b])
            a, b = b, a
        out.append(a[wet].copy())
    return c0[wet], exact[wet], out


@pytest.mark.parametrize("cu,cv", [(0.25, 0.125), (0.25, 0.25)])
def test_gaussian_2d_beats_limited_and_stays_in_range(cu, cv):
    """two dimensions get only these two measured runs: L1 below section 6.11's, no excursion from the initial range beyond
    steps * 32 ulp"""
    steps = 96
    c0, exact, runs = carry_2d(cu, cv, steps=steps)
    l1, over, _, span = _report("2-D gaussian at (%g, %g)" % (cu, cv), steps, c0, exact, runs)
    assert l1[2] < l1[1]
    assert over[2] <= steps * 32 * ULP * span, over[2] / ULP
