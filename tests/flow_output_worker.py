"""One rank of the N-process test of psy.flow_output on a decomposed grid (tests/test_a_flow_output_ranks_gpu.py).  The ranks
are separate processes sharing device 0 in mailbox mode; the decomposition (halo_width = 1) is the product's own.

Every rank holds its window of one random -1 / 0 / 1 mask and of the four random flow arrays of the UNDIVIDED domain, and
has the six arrays of tests/flow_output_numpy.py for the undivided domain next to it.  The halo cells that belong to a
neighbour start out wrong on purpose -- land in the mask, NaN in un and vn -- and are fetched by grid_mod.exchange_mask_halos
and field.halo_exchange, corners included: VORT reads the mask and vn one cell to the north-east.  psy.flow_output is not
collective; every rank's internal region must hold the undivided domain's bits for all six outputs, in SET and after two ADD
calls, and its halos the sentinel.  The same under a mask that leaves rank 0 all land.

    RANK=r WORLD_SIZE=n MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/flow_output_worker.py NX NY NDX NDY
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NX, NY, NDX, NDY = (int(a) for a in sys.argv[1:5])
SEED = 20261022
DXY = 1000.0
SENTINEL = -7.0
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

dist.init_process_group("gloo", rank=rank, world_size=world)
import dl_esm_inf_amd as D  # noqa: E402
import flow_output_numpy as ON  # noqa: E402
import tracer_cases as TC  # noqa: E402
from dl_esm_inf_amd import grid_mod  # noqa: E402
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


rng = np.random.default_rng(SEED)
GM = TC.random_mask(rng, GNY, GLD)
GH = _host_inputs(rng, GM.shape)
GD = np.full((GNY, GLD), DXY)             # dx_v and dy_u of the undivided domain
NAMES = ("un", "vn", "ht", "sshn_t")      # psy.flow_output's order
T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
PTS = dict(un=U, vn=V, ht=T, sshn_t=T)


def case(what, user):
    os.environ["DL_ESM_ALIGNMENT"] = "64"
    g = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
    g.decompose(NX, NY, ndomains=world, ndomainx=NDX, ndomainy=NDY)
    os.environ.pop("DL_ESM_ALIGNMENT", None)
    it = g.subdomain.internal
    ox = g.subdomain.glob.xstart - it.xstart + 1      # global index of local (0-based) column 0
    oy = g.subdomain.glob.ystart - it.ystart + 1
    xs, xe, ys, ye = it.xstart, it.xstop, it.ystart, it.ystop

    def local(glob, shape=None):
        """this tile's window of a global array, of the grid's extents or `shape` (cells beyond the global array: 0)"""
        ny, nx = shape or (g.ny, g.nx)
        out = np.zeros((ny, nx), dtype=glob.dtype)
        y0, x0 = max(0, -oy), max(0, -ox)
        y1, x1 = min(ny, GNY - oy), min(nx, GLD - ox)
        out[y0:y1, x0:x1] = glob[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        return out

    def foreign(shape):
        """the cells of the tile's one-cell ring that are internal cells of the undivided domain: a neighbour's"""
        ny, nx = shape
        jj, ii = np.mgrid[0:ny, 0:nx]
        ring = ((jj == ys - 2) | (jj == ye) | (ii == xs - 2) | (ii == xe)) & (jj >= ys - 2) & (jj <= ye) & (ii >= xs - 2) & (ii <= xe)
        gj, gi = jj + oy, ii + ox
        return ring & (gj >= 1) & (gj <= NY) & (gi >= 1) & (gi <= NX)

    # the mask: the neighbours' cells of the ring start as land and come over the wire, corners included
    shape = (it.ystop + 1, it.xstop + 1)
    window = local(user, shape)
    start = window.copy()
    theirs = foreign(shape)
    start[theirs] = 0
    D.grid_init(g, DXY, DXY, tmask=start)
    grid_mod.exchange_mask_halos(g)
    inside = (slice(ys - 2, ye + 1), slice(xs - 2, xe + 1))               # the tile and its one-cell ring
    if not np.array_equal(g.tmask_device.cpu().numpy()[inside], local(user)[inside]):
        error(f"{what}: after exchange_mask_halos the mask is not this rank's window of the global mask")
    if world > 1 and not theirs.any():
        error(f"{what}: no halo cell belongs to a neighbour")
    if NDX > 1 and NDY > 1 and not theirs[[ys - 2, ys - 2, ye, ye], [xs - 2, xe, xs - 2, xe]].any():
        error(f"{what}: no corner of the ring belongs to a neighbour")
    F = {}
    for k in NAMES:
        f = D.r2d_field(g, PTS[k])
        a = local(GH[k])
        if k in ("un", "vn"):
            a[foreign(a.shape)] = np.nan
        f.set_data(a)
        if k in ("un", "vn"):
            f.halo_exchange(depth=1)
        F[k] = f
    torch.cuda.synchronize()
    outs = []
    for _ in range(ON.COUNT):
        f = D.r2d_field(g, T)
        f.set_data(np.full((g.ny, g.nx), SENTINEL))
        outs.append(f)
    named = dict(zip(ON.NAMES, outs))
    want = [np.full((GNY, GLD), SENTINEL) for _ in range(ON.COUNT)]
    flow = [GH[k] for k in NAMES]
    mine = np.zeros((g.ny, g.nx), dtype=bool)
    mine[ys - 1:ye, xs - 1:xe] = True

    def compare(step):
        for k in range(ON.COUNT):
            got = outs[k].get_data()
            ref = local(want[k])
            if not ON.same(got[mine], ref[mine]):
                n = int(np.count_nonzero((got != ref) & ~(np.isnan(got) & np.isnan(ref)) & mine))
                error(f"{what}: {step}: {ON.NAMES[k]}: {n} internal cells differ from the undivided domain")
            if not (got[~mine] == SENTINEL).all():
                error(f"{what}: {step}: {ON.NAMES[k]}: a halo cell was written")

    D.psy.flow_output(*[F[k] for k in NAMES], **named)
    ON.flow_output(ON.SET, 0.0, GBOX, user, GD, GD, *flow, want)
    compare("set")
    for _ in range(2):
        D.psy.flow_output(*[F[k] for k in NAMES], **named, weight=0.375)
        ON.flow_output(ON.ADD, 0.375, GBOX, user, GD, GD, *flow, want)
    compare("add")
    wet_here = int((local(user)[mine] > 0).sum())
    vort_here = int(local(ON.written(user, GBOX, ON.VORT).astype(np.int32))[mine].sum())
    print(f"rank {rank} {what}: {wet_here} wet cells, {vort_here} with a vorticity", flush=True)
    return (ox, oy, (xs, xe, ys, ye)), wet_here, vort_here


tile, wet, vort = case("whole", GM)
if wet < NX * NY // (3 * world) or vort < 20:
    error(f"whole: {wet} wet cells, {vort} with a vorticity")

# a mask that leaves rank 0 all land: it writes nothing, its neighbours read land across the boundary
tiles = [None] * world
dist.all_gather_object(tiles, tile)
tx, ty, (xs, xe, ys, ye) = tiles[0]
GDRY = GM.copy()
GDRY[ys - 1 + ty:ye + ty, xs - 1 + tx:xe + tx] = 0
_, dry, _ = case("rank 0 all land", GDRY)
if (dry != 0) if rank == 0 else (dry == 0):
    error(f"rank 0 all land: {dry} wet cells")

if L.dlesm_wait_timed_out(0):
    error("a device-side wait gave up")
t = torch.tensor([errors])
dist.all_reduce(t)
dist.barrier()
print(f"rank {rank}: {NDX}x{NDY} tiles of {NX}x{NY}, errors {errors} (all ranks {int(t.item())})", flush=True)
D.parallel_finalise()
dist.destroy_process_group()
sys.exit(1 if int(t.item()) else 0)
