"""Test helpers of the tracer transport tests: the flow and tracer inputs the CPU and GPU tests
share, the special-value case of the three schemes (sections 6.10-6.12), the land overwrites of the invariance tests, and a
NEMOLite2D-class CPU time step built from the existing restatements (oracle_lib continuity, momentum_numpy, open_bc_numpy)
that carries tracers with tracer_numpy.
Nothing here needs a GPU.
"""
import math

import numpy as np

import momentum_numpy as M
import open_bc_numpy as B
import oracle_lib as O
import tracer_hancock_numpy as TH
import tracer_muscl_numpy as TM
import tracer_numpy as TN
from nemolite_boxes import METRICS, MOM, PRM, SPECIAL, _host_inputs, host_grid, is_subnormal

FLOW = ("un", "vn", "hu", "hv", "ht", "sshn_t", "sshn_u", "sshn_v", "ssha")     # the C entry's order, after tmask and area_t
RDT = 600.0
SENTINEL = -7.0
LAND_FILLS = (np.nan, 1e300, -3.0)


def random_mask(rng, ny, ld):
    return B.repair(rng.choice(np.array([-1, 0, 1, 1, 1], dtype=np.int32), size=(ny, ld)))


def flow_inputs(rng, tm):
    """(area_t, flow dict in FLOW's names): non-uniform metrics, velocities with signed zeros, ssha of the size of sshn_t"""
    G = host_grid(rng, tm)
    H = _host_inputs(rng, tm.shape)
    H["ssha"] = 0.1 * rng.normal(size=tm.shape)
    return G["area_t"], {k: H[k] for k in FLOW}


def tracers(rng, shape, k):
    """k tracers of different data, and sentinel-filled outputs"""
    return [float(n + 1) + rng.random(shape) for n in range(k)], [np.full(shape, SENTINEL) for _ in range(k)]


PATCH = (slice(3, 7), slice(8, 40))             # special_case's patch of unit weights: rows 3..6, columns 8..39 (0-based)
ONE_BELOW = float(np.nextafter(1.0, 0.0))
PATCH_VELOCITIES = np.array([1.0, ONE_BELOW, 0.5, 0.0, -0.0, -1.0, 2.0, -ONE_BELOW])


def _sprinkle(rng, a, share):
    """nemolite_boxes.SPECIAL drawn into `share` of the cells of a"""
    pick = rng.random(a.shape) < share
    a[pick] = rng.choice(SPECIAL, size=int(pick.sum()))


def special_case(seed, ld, ny, rdt):
    """(tm, area_t, H, c_in, c_out) with four tracers, for arrays of at least 9 rows and 42 columns: random_mask and
    flow_inputs, then the values at which the arithmetic of sections 6.10-6.12 has an edge, in wet cells:
      * nemolite_boxes.SPECIAL (subnormals, signed zeros, infinities, NaN of both signs, 1e300, 1e154) in 2 % of un and vn,
        in 0.5 % of every other flow array and in 0.4 % of area_t -- an area of 0 makes q and w infinite;
      * ssha = -ht on 1 % of the wet cells and sshn_t = -ht on another 1 %: h_new == 0 and h_old == 0 (and one cell of each
        kind in PATCH's last column, so that a small box holds them whatever the random picks hit);
      * PATCH, all wet, with area_t = rdt, ht = hu = hv = 1 and every surface 0, so that w == 1 exactly and a face's Courant
        number is the magnitude of its velocity, drawn from PATCH_VELOCITIES: 1, one ulp below 1, 0.5, 0 and 2;
      * tracer 0: multiples of 1/2 in 0 .. 2, so that every tie of the limiter occurs (a == b, a == 0, a == -b and
        2|a| == |a+b|/2); tracer 1: 1 + random with SPECIAL in 2 % of the cells; tracer 2: multiples of 2.5e-310, so that its
        slopes are subnormal; tracer 3: of the order of 1e300, so that its fluxes overflow.
    The outputs hold SENTINEL."""
    rng = np.random.default_rng(seed)
    tm = random_mask(rng, ny, ld)
    area_t, H = flow_inputs(rng, tm)
    shape = tm.shape
    for k in ("un", "vn"):
        _sprinkle(rng, H[k], 0.02)
    for k in ("sshn_u", "sshn_v", "hu", "hv", "ht", "sshn_t", "ssha"):
        _sprinkle(rng, H[k], 0.005)
    _sprinkle(rng, area_t, 0.004)
    pick = rng.random(shape)
    new, old = (pick < 0.01) & (tm > 0), (pick >= 0.01) & (pick < 0.02) & (tm > 0)
    H["ssha"][new] = -H["ht"][new]
    H["sshn_t"][old] = -H["ht"][old]
    tm[PATCH] = 1
    area_t[PATCH] = float(rdt)
    for k in ("ht", "hu", "hv"):
        H[k][PATCH] = 1.0
    for k in ("sshn_t", "sshn_u", "sshn_v", "ssha"):
        H[k][PATCH] = 0.0
    for k in ("un", "vn"):
        H[k][PATCH] = rng.choice(PATCH_VELOCITIES, size=H[k][PATCH].shape)
    H["ssha"][PATCH][0, -1] = -1.0                 # whatever the random picks hit: h_new == 0 in one cell of the patch ...
    H["sshn_t"][PATCH][2, -1] = -1.0               # ... and h_old == 0 (an infinite w) in another
    c_in = [0.5 * rng.integers(0, 5, shape), 1.0 + rng.random(shape), 2.5e-310 * rng.integers(-3, 4, shape),
            1e300 * (rng.random(shape) - 0.5)]
    _sprinkle(rng, c_in[1], 0.02)
    return tm, area_t, H, c_in, [np.full(shape, SENTINEL) for _ in range(4)]


# the three schemes: (C entry, HOOK key, array restatement, scalar restatement)
SCHEMES = {
    "upwind": ("dlesm_tracer_step_f64", "tracer_kernel", TN.tracer_step, TN.tracer_step_scalar),
    "muscl": ("dlesm_tracer_step_muscl_f64", "tracer_muscl_kernel", TM.tracer_step_muscl, TM.tracer_step_muscl_scalar),
    "hancock": ("dlesm_tracer_step_hancock_f64", "tracer_hancock_kernel", TH.tracer_step_hancock,
                TH.tracer_step_hancock_scalar),
}
# 260: three wave tiles of the limited schemes with both seams in the box; 131: the odd pitch; 130 x 9: a sub-box
SPECIAL_SHAPES = [(260, 12, (2, 259, 2, 11)), (131, 10, (2, 130, 2, 9)), (130, 9, (5, 100, 3, 8))]
RDT_BIG = 3.0e6                                   # puts the random faces on both sides of a Courant number of 1
_SPECIAL = {}


def special_host(ld, ny, rdt):
    """special_case of the shape with the modules' seeding rule, made once and never modified"""
    key = (ld, ny, float(rdt))
    if key not in _SPECIAL:
        _SPECIAL[key] = special_case(ld * 7 + ny, ld, ny, rdt)
    return _SPECIAL[key]


def special_reference(scheme, ld, ny, box, rdt, k=4):
    """what the scheme's array restatement leaves of the first k tracers of special_host; made once, never modified"""
    key = (scheme, ld, ny, box, float(rdt), k)
    if key not in _SPECIAL:
        tm, area_t, H, c_in, c_out = special_host(ld, ny, rdt)
        want = [a.copy() for a in c_out[:k]]
        SCHEMES[scheme][2](rdt, box, tm, area_t, *[H[n] for n in FLOW], c_in[:k], want)
        _SPECIAL[key] = want
    return _SPECIAL[key]


def written(tm, box):
    """the cells a tracer step writes: the wet cells of the box"""
    xs, xe, ys, ye = box
    out = np.zeros(tm.shape, dtype=bool)
    out[ys - 1:ye, xs - 1:xe] = tm[ys - 1:ye, xs - 1:xe] > 0
    return out


def holds_specials(outs, cells):
    """(an infinity, a NaN, a subnormal) among `cells` of the arrays `outs`"""
    v = np.concatenate([o[cells] for o in outs])
    return bool(np.isinf(v).any()), bool(np.isnan(v).any()), bool(is_subnormal(v).any())


def reference(rdt, box, tm, area_t, H, c_in, c_out):
    """c_out as tracer_numpy leaves it (copies)"""
    want = [a.copy() for a in c_out]
    TN.tracer_step(rdt, box, tm, area_t, *[H[k] for k in FLOW], c_in, want)
    return want


def land_faces(tm):
    """(u faces, v faces) that touch land: the face (i, j) lies between T(i, j) and T(i+1, j) / T(i, j+1); the last column /
    row has no cell beyond it and counts as touching land only through its own cell"""
    land = tm == 0
    fu, fv = land.copy(), land.copy()
    fu[:, :-1] |= land[:, 1:]
    fv[:-1, :] |= land[1:, :]
    return fu, fv


def overwrite_land(tm, H, c_in, fill):
    """copies of the flow and the tracers with `fill` in every tracer's land cells and NaN in un / vn on every face that
    touches land"""
    fu, fv = land_faces(tm)
    H2 = {k: v.copy() for k, v in H.items()}
    H2["un"][fu] = np.nan
    H2["vn"][fv] = np.nan
    c2 = [c.copy() for c in c_in]
    for c in c2:
        c[tm == 0] = fill
    return H2, c2


# ---- a tidal open channel ---------------------------------------------------------------------------------------------
def channel_user_mask(nx, ny):
    """the user mask (ny + 2, nx + 2) of an open channel: open first and last internal columns, two land rows north and south"""
    user = np.ones((ny + 2, nx + 2), dtype=np.int32)
    user[:, 0] = user[:, -1] = 0
    user[:, 1] = user[:, nx] = -1
    user[:2, :] = 0
    user[-2:, :] = 0
    return user


def uniform_grid(tm, dxy=1000.0, lat=50.0):
    """a host grid namespace of uniform metrics over the mask tm, as grid_init makes it"""
    G = {"tmask": np.ascontiguousarray(tm, dtype=np.int32)}
    for name in METRICS:
        G[name] = np.full(tm.shape, float(dxy * dxy if name.startswith("area") else dxy))
    G["fcor_u"] = M.coriolis(np.full(tm.shape, lat), 7.292116e-5, math.pi / 180.0)
    G["fcor_v"] = G["fcor_u"].copy()
    return M.SimpleNamespace(**G)


STATE = ("ssha", "sshn_t", "sshn_u", "sshn_v", "ssha_u", "ssha_v", "un", "vn", "ua", "va", "ht", "hu", "hv")
ROTATE = (("un", "ua"), ("vn", "va"), ("sshn_t", "ssha"), ("sshn_u", "ssha_u"), ("sshn_v", "ssha_v"))


# Continuity's fluxes carry no face length, so a tracer's Courant number is |r| rdt / (area_t h): a 10 m mesh, a 1 s step
# and a 3 m/s current give 0.03, with the surface waves (g h rdt^2 / dx^3 = 0.1) and the viscous term (visc rdt / dx^2 =
# 0.01) well inside their stability bounds.
CHANNEL_DXY = 10.0
CHANNEL_PRM = (1.0, 0.00015, 1.0, 9.80665)    # rdt, cbfr, visc, g
CHANNEL_TIDE = (0.1, 2.0 * math.pi / 60.0)    # amplitude, omega


def channel_state(tm, nx, ny, bump=0.5, current=3.0):
    """a channel 10 m deep with a bump of the surface and a uniform current along it on every u face between two cells that
    are not land (in through the open west column, out through the east one)"""
    shape = tm.shape
    H = {k: np.zeros(shape) for k in STATE}
    for k in ("ht", "hu", "hv"):
        H[k][:] = 10.0
    jj, ii = np.mgrid[0:shape[0], 0:shape[1]]
    H["sshn_t"][:] = bump * np.exp(-((ii - 0.6 * nx) ** 2 + (jj - 0.5 * ny) ** 2) / (2 * (nx / 10.0) ** 2))
    face = tm != 0
    face[:, :-1] &= tm[:, 1:] != 0
    face[:, -1] = False
    H["un"][face] = current
    return H


def channel_tracers(tm, seed=11):
    """(c_in, c_out) of two tracers, both buffers alike: c = 1 everywhere, and a dye in [0, 1] with the boundary value 0.5
    in the open cells"""
    ones = np.ones(tm.shape)
    dye = np.random.default_rng(seed).random(tm.shape)
    dye[tm < 0] = 0.5
    return [ones.copy(), dye.copy()], [ones.copy(), dye.copy()]


def cpu_step(G, box, H, ssh_bc, c_in, c_out, prm=PRM):
    """one NEMOLite2D-class step on the host (DESIGN.md section 6.7's order; ssh_bc None: a closed basin), then the tracers
    carried from c_in to c_out with the level-n flow and the new ssha.  Rotates nothing."""
    rdt, ld = prm[0], G.tmask.shape[1]
    hp = M.params(*prm)
    O.continuity_slabs(rdt, ld, box, H["sshn_t"], H["sshn_u"], H["sshn_v"], H["hu"], H["hv"], H["un"], H["vn"], G.area_t,
                       H["ssha"])
    if ssh_bc is not None:
        B.bc_ssh(box, G.tmask, ssh_bc, H["ssha"])
    M.next_sshu(box, G.tmask, G.area_t, G.area_u, H["ssha"], H["ssha_u"])
    M.next_sshv(box, G.tmask, G.area_t, G.area_v, H["ssha"], H["ssha_v"])
    M.momentum(hp, G, box, box, *[H[k] for k in MOM], H["ua"], H["va"])
    if ssh_bc is not None:
        B.flather_u(hp, box, G.tmask, H["hu"], H["sshn_u"], H["sshn_t"], H["ua"])
        B.flather_v(hp, box, G.tmask, H["hv"], H["sshn_v"], H["sshn_t"], H["va"])
    TN.tracer_step(rdt, box, G.tmask, G.area_t, *[H[k] for k in FLOW], c_in, c_out)


def rotate(H):
    for a, b in ROTATE:
        H[a], H[b] = H[b], H[a]


def cfl(rdt, box, G, H):
    """max over the wet cells of the box of |r| q / h_new, r any of the four face transports"""
    xs, xe, ys, ye = box

    def S(a, di=0, dj=0):
        return a[ys - 1 + dj:ye + dj, xs - 1 + di:xe + di]
    with np.errstate(all="ignore"):
        r = [np.abs((S(H["sshn_u"], d, 0) + S(H["hu"], d, 0)) * S(H["un"], d, 0)) for d in (0, -1)]
        r += [np.abs((S(H["sshn_v"], 0, d) + S(H["hv"], 0, d)) * S(H["vn"], 0, d)) for d in (0, -1)]
        x = np.maximum.reduce(r) * (rdt / S(G.area_t)) / (S(H["ht"]) + S(H["ssha"]))
    return float(x[S(G.tmask) > 0].max())
