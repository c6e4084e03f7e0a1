"""One rank of the N-process test of psy.flow_courant / psy.flow_courant_check on a decomposed grid
(tests/test_a_flow_courant_ranks_gpu.py).  The ranks are separate processes sharing device 0 in mailbox mode; the
decomposition (halo_width = 1) is the product's own.

Every rank holds its window -- depth-1 halos included -- of one random -1 / 0 / 1 mask and of the four random flow arrays of
the UNDIVIDED domain, on a grid of uniform cells, and has the record of tests/flow_courant_numpy.py for the undivided domain
next to it.  On every rank psy.flow_courant must give that record's extremes and counts exactly, and as locations the lowest
rank that owns a cell with the extreme and the local (i, j) of its first such cell (the undivided domain's linear index mapped
to its owner) -- at an rdt below the limits and at one that puts cells on both sides of the gravity-wave limit;
flow_courant_check must return at the first and raise on every rank at the second, naming the count, the owner and the cell.
The same under a mask that leaves rank 0 without a wet cell, and with a negative depth in one cell of the last rank
(invalid == 1 everywhere).

    RANK=r WORLD_SIZE=n MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/flow_courant_worker.py NX NY NDX NDY
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NX, NY, NDX, NDY = (int(a) for a in sys.argv[1:5])
SEED = 20261021
DXY = 1000.0
G, VISC = 9.80665, 100.0
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

dist.init_process_group("gloo", rank=rank, world_size=world)
import dl_esm_inf_amd as D  # noqa: E402
import flow_courant_numpy as FN  # noqa: E402
import tracer_cases as TC  # noqa: E402
from nemolite_boxes import _host_inputs  # noqa: E402

torch.cuda.set_device(0)
L = D._cabi.lib()
L.dlesm_set_tuning(b"dm_wait_seconds", 30)         # a protocol error must end in words, not in a hung box
D.parallel_init(rank, world, transport="mailbox")

GNY, GLD = NY + 2, NX + 2                 # the undivided domain and its one-cell ring
GBOX = (2, NX + 1, 2, NY + 1)             # its internal region, 1-based
errors = 0


def error(msg):
    global errors
    errors += 1
    print(f"ERROR rank {rank}: {msg}", flush=True)


def make_grid(user):
    """(grid, ox, oy): the decomposed grid whose mask is this rank's window of `user`; ox, oy = the global index of local
    (0-based) column / row 0"""
    os.environ["DL_ESM_ALIGNMENT"] = "64"
    g = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
    g.decompose(NX, NY, ndomains=world, ndomainx=NDX, ndomainy=NDY)
    os.environ.pop("DL_ESM_ALIGNMENT", None)
    it = g.subdomain.internal
    ox = g.subdomain.glob.xstart - it.xstart + 1
    oy = g.subdomain.glob.ystart - it.ystart + 1
    D.grid_init(g, DXY, DXY, tmask=local(user, g, ox, oy, shape=(it.ystop + 1, it.xstop + 1)))
    return g, ox, oy


def local(glob, g, ox, oy, shape=None):
    """this tile's window of a global array, of the grid's extents or `shape` (cells beyond the global array: 0)"""
    ny, nx = shape or (g.ny, g.nx)
    out = np.zeros((ny, nx), dtype=glob.dtype)
    y0, x0 = max(0, -oy), max(0, -ox)
    y1, x1 = min(ny, GNY - oy), min(nx, GLD - ox)
    out[y0:y1, x0:x1] = glob[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


rng = np.random.default_rng(SEED)
GM = TC.random_mask(rng, GNY, GLD)
GH = _host_inputs(rng, GM.shape)
GD = np.full((GNY, GLD), DXY)             # dx_t and dy_t of the undivided domain
NAMES = ("un", "vn", "ht", "sshn_t")      # psy.flow_courant's order
T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
PTS = dict(un=U, vn=V, ht=T, sshn_t=T)


def case(what, user, H):
    """one mask and one flow: the grid, the fields, the checks at both rdt"""
    g, ox, oy = make_grid(user)
    it = g.subdomain.internal
    tiles = [None] * world                             # (ox, oy, internal box) of every rank
    dist.all_gather_object(tiles, (ox, oy, (it.xstart, it.xstop, it.ystart, it.ystop)))
    inside = (slice(it.ystart - 2, it.ystop + 1), slice(it.xstart - 2, it.xstop + 1))     # the tile and its one-cell ring
    if not np.array_equal(g.tmask_device.cpu().numpy()[inside], local(user, g, ox, oy)[inside]):
        error(f"{what}: the grid's mask is not this rank's window of the global mask")
    if not ((g.dx_t_device.cpu().numpy()[inside] == DXY).all() and (g.dy_t_device.cpu().numpy()[inside] == DXY).all()):
        error(f"{what}: dx_t / dy_t")
    F = []
    for k in NAMES:
        f = D.r2d_field(g, PTS[k])
        f.set_data(local(H[k], g, ox, oy))
        F.append(f)

    def owner_of(gj, gi):
        """(1-based rank, local 1-based (i, j)) of the cell at index [gj, gi] of the undivided array"""
        for r, (tx, ty, (xs, xe, ys, ye)) in enumerate(tiles):
            i, j = gi - tx + 1, gj - ty + 1
            if xs <= i <= xe and ys <= j <= ye:
                return r + 1, i, j
        raise AssertionError((gj, gi))

    def place(x, has, top):
        """(rank, i, j) of the lowest rank that owns a cell with x == top, and of its first such cell"""
        if not has.any():
            return None
        at = [owner_of(j + 1, i + 1) for j, i in np.argwhere(has & (x == top))]       # the box starts at [1, 1]
        return min(at, key=lambda a: (a[0], a[2], a[1]))

    flow = [H[k] for k in NAMES]
    unit = FN.flow_courant(1.0, G, VISC, GBOX, user, GD, GD, *flow)
    top = max(unit.gravity_max / 1.0, unit.advective_max / 1.0, unit.viscous_max / 0.25)
    rdts = [0.5 / top, 1.02 / top] if top > 0.0 else [1.0]
    for n, rdt in enumerate(rdts):
        want = FN.flow_courant(rdt, G, VISC, GBOX, user, GD, GD, *flow)
        c = FN.cells(rdt, G, VISC, GBOX, user, GD, GD, *flow)
        ok = c["wet"] & ~c["bad"]
        want_at = (place(c["gw"], ok, want.gravity_max), place(c["adv"], ok, want.advective_max),
                   place(c["vis"], ok, want.viscous_max), place(c["d"], ok, want.depth_min))
        # the undivided domain's own linear indices name cells that attain the extremes, too
        for index, x, top_x in zip(want[4:8], (c["gw"], c["adv"], c["vis"], c["d"]), want[:4]):
            if index >= 0 and x[index // GLD - 1, index % GLD - 1] != top_x:
                error(f"{what}: the undivided record's index {index}")
        r = D.psy.flow_courant(rdt, *F, g=G, visc=VISC)
        print(f"rank {rank} {what} rdt {rdt!r}: got {r} want {want} at {want_at}", flush=True)
        if tuple(r[:4]) + tuple(r[8:14]) != tuple(want[:4]) + tuple(want[8:14]):
            error(f"{what}: {r}, undivided domain {want}")
        if tuple(r[4:8]) != want_at:
            error(f"{what}: locations {r[4:8]}, undivided domain {want_at}")
        if r.rdt_limit != FN.rdt_limit(rdt, want):
            error(f"{what}: rdt_limit {r.rdt_limit!r}")
        over = want.invalid or want.gravity_over or want.advective_over or want.viscous_over or want.shallow
        try:
            if D.psy.flow_courant_check(rdt, *F, g=G, visc=VISC) != r:
                error(f"{what}: flow_courant_check returns another result")
            if over:
                error(f"{what}: flow_courant_check did not raise")
        except D.DlesmError as e:
            word = ("invalid: %d wet" % want.invalid if want.invalid else "gravity_over: %d wet" % want.gravity_over)
            at = None if want.invalid else want_at[0]
            where = "" if at is None else "(i, j) = (%d, %d) on rank %d" % (at[1], at[2], at[0])
            if not over or word not in str(e) or where not in str(e):
                error(f"{what}: flow_courant_check message: {e}")
        if n == 0 and over and not want.invalid:
            error(f"{what}: the small rdt reaches a limit")
        if n == 1 and not 0 < want.gravity_over < want.wet - want.invalid:
            error(f"{what}: the large rdt leaves no cell on one side of the gravity-wave limit: {want}")
    return tiles, want


tiles, want = case("whole", GM, GH)
if want.wet < NX * NY // 3 or want.invalid:
    error(f"whole: {want}")

# a mask that leaves rank 0 without a wet cell: every rank still has the record of the whole domain
GDRY = GM.copy()
tx, ty, (xs, xe, ys, ye) = tiles[0]
GDRY[ys - 1 + ty:ye + ty, xs - 1 + tx:xe + tx] = 0
_, dry = case("rank 0 dry", GDRY, GH)
if dry.wet >= want.wet or dry.wet == 0:
    error(f"rank 0 dry: {dry}")

# a negative depth in a wet cell of the last rank: invalid on every rank
tx, ty, (xs, xe, ys, ye) = tiles[world - 1]
cells = np.argwhere(GM[ys - 1 + ty:ye + ty, xs - 1 + tx:xe + tx] > 0)
H2 = {k: v.copy() for k, v in GH.items()}
H2["ht"][ys - 1 + ty + cells[0][0], xs - 1 + tx + cells[0][1]] = -20.0
_, sick = case("one negative depth", GM, H2)
if sick.invalid != 1:
    error(f"one negative depth: {sick}")

if L.dlesm_wait_timed_out(0):
    error("a device-side wait gave up")
t = torch.tensor([errors])
dist.all_reduce(t)
dist.barrier()
print(f"rank {rank}: {NDX}x{NDY} tiles of {NX}x{NY}, errors {errors} (all ranks {int(t.item())})", flush=True)
D.parallel_finalise()
dist.destroy_process_group()
sys.exit(1 if int(t.item()) else 0)
