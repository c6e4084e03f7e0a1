"""One rank of the N-process test of field_stats / psy.run_health on a decomposed grid (tests/test_a_field_stats_ranks_gpu.py).
The ranks are separate processes sharing device 0 in mailbox mode; the decomposition (halo_width = 1) is the product's own.

Every rank holds its window of one random field in [-0.5, 0.5) and of one random -1 / 0 / 1 mask of the UNDIVIDED domain, and
has numpy's numbers of the undivided domain next to it.  On every rank field_stats must give those: min, max, count and
nonfinite exactly, sum and sumsq within n 2^-52 fsum(|x|) resp. n 2^-52 fsum(x^2) (the worst case of any summation order,
see tests/test_gpu_field_stats.py) -- unmasked, masked, with a NaN in a cell of the last rank (nonfinite == 1 everywhere),
and under a mask that leaves rank 0 without a wet cell.  run_health must raise on every rank and name the rank that owns the
offending cell and its local (i, j): for the NaN, and for a value beyond max_abs on rank 0.

    RANK=r WORLD_SIZE=n MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/field_stats_worker.py NX NY NDX NDY
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NX, NY, NDX, NDY = (int(a) for a in sys.argv[1:5])
SEED = 20261017
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

dist.init_process_group("gloo", rank=rank, world_size=world)
import dl_esm_inf_amd as D  # noqa: E402

torch.cuda.set_device(0)
L = D._cabi.lib()
L.dlesm_set_tuning(b"dm_wait_seconds", 30)         # a protocol error must end in words, not in a hung box
D.parallel_init(rank, world, transport="mailbox")

GNY, GLD = NY + 2, NX + 2                 # the undivided domain and its one-cell ring
errors = 0


def error(msg):
    global errors
    errors += 1
    print(f"ERROR rank {rank}: {msg}", flush=True)


os.environ["DL_ESM_ALIGNMENT"] = "64"
g = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
g.decompose(NX, NY, ndomains=world, ndomainx=NDX, ndomainy=NDY)
os.environ.pop("DL_ESM_ALIGNMENT", None)
D.grid_init(g, 1.0, 1.0)
it = g.subdomain.internal
ox = g.subdomain.glob.xstart - it.xstart + 1      # global index of local (0-based) column 0
oy = g.subdomain.glob.ystart - it.ystart + 1
tiles = [None] * world                             # (ox, oy, internal box) of every rank
dist.all_gather_object(tiles, (ox, oy, (it.xstart, it.xstop, it.ystart, it.ystop)))


def local(glob, dtype=np.float64):
    """this tile's window of a global array (cells beyond the global array: 0)"""
    out = np.zeros((g.ny, g.nx), dtype=dtype)
    y0, x0 = max(0, -oy), max(0, -ox)
    y1, x1 = min(g.ny, GNY - oy), min(g.nx, GLD - ox)
    out[y0:y1, x0:x1] = glob[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


def owner_of(gj, gi):
    """(0-based rank, local 1-based (i, j)) of the cell at index [gj, gi] of the undivided array"""
    for r, (tx, ty, (xs, xe, ys, ye)) in enumerate(tiles):
        i, j = gi - tx + 1, gj - ty + 1
        if xs <= i <= xe and ys <= j <= ye:
            return r, (i, j)
    raise AssertionError((gj, gi))


def want_of(H, M=None):
    x = H[1:NY + 1, 1:NX + 1]
    x = x[M[1:NY + 1, 1:NX + 1] > 0] if M is not None else x.ravel()
    fin = np.isfinite(x)
    xf = x[fin]
    return (xf.min() if xf.size else math.inf, xf.max() if xf.size else -math.inf, math.fsum(xf), math.fsum(xf * xf), x.size,
            int((~fin).sum()), math.fsum(np.abs(xf)), xf.size)


def compare(st, want, what):
    mn, mx, s, q, cnt, nf, sabs, n = want
    print(f"rank {rank} {what}: got {st!r} want {want}", flush=True)
    if (st.min, st.max, st.count, st.nonfinite) != (mn, mx, cnt, nf):
        error(f"{what}: {st!r}, undivided domain {want}")
    if not abs(st.sum - s) <= n * 2.0 ** -52 * sabs:
        error(f"{what}: sum {st.sum!r}, undivided domain {s!r}")
    if not abs(st.sumsq - q) <= n * 2.0 ** -52 * q:
        error(f"{what}: sumsq {st.sumsq!r}, undivided domain {q!r}")


rng = np.random.default_rng(SEED)
GH = rng.random((GNY, GLD)) - 0.5
GM = rng.integers(-1, 2, size=(GNY, GLD)).astype(np.int32)
x = D.r2d_field(g, D.GO_T_POINTS)
assert x.internal.box() == (it.xstart, it.xstop, it.ystart, it.ystop)
x.set_data(local(GH))
m = torch.from_numpy(local(GM, np.int32)).cuda()

st = D.field_stats([x, x], [None, m])
compare(st[0], want_of(GH), "unmasked")
compare(st[1], want_of(GH, GM), "masked")
if st[0].count != NX * NY:
    error(f"count {st[0].count}")
if D.psy.run_health([x], ["x"], max_abs=[0.5])[0].as6() != st[0].as6():
    error("run_health on a healthy field does not return the stats")

# a mask that leaves rank 0 without a wet cell: every rank still has the numbers of the whole domain
GD = np.ones((GNY, GLD), dtype=np.int32)
tx, ty, (xs, xe, ys, ye) = tiles[0]
GD[ys - 1 + ty:ye + ty, xs - 1 + tx:xe + tx] = 0
md = torch.from_numpy(local(GD, np.int32)).cuda()
std = D.field_stats([x], md)[0]
compare(std, want_of(GH, GD), "rank 0 dry")
if std.count != NX * NY - (xe - xs + 1) * (ye - ys + 1):
    error(f"rank 0 dry: count {std.count}")

# a value beyond max_abs in a cell of rank 0: every rank raises and names rank 1 (1-based) and the cell
gj, gi = 3, 4
who, cell = owner_of(gj, gi)
assert who == 0
GH[gj, gi] = 7.0
x.set_data(local(GH))
try:
    D.psy.run_health([x], ["ssh"], max_abs=[1.0])
    error("run_health did not raise on a value beyond max_abs")
except D.DlesmError as e:
    if "field ssh" not in str(e) or f"(i, j) = ({cell[0]}, {cell[1]}) on rank 1" not in str(e):
        error(f"run_health message: {e}")
if D.psy.run_health([x], ["ssh"], masks=md, max_abs=[1.0])[0].max >= 0.5:      # the cell is dry under that mask
    error("a dry cell counted")
GH[gj, gi] = 0.25

# a NaN in a cell of the last rank: nonfinite == 1 on all ranks, run_health raises on all ranks and names the owner
gj, gi = NY - 2, NX - 3
who, cell = owner_of(gj, gi)
assert who == world - 1
GH[gj, gi] = np.nan
x.set_data(local(GH))
st = D.field_stats([x])[0]
compare(st, want_of(GH), "one NaN")
if st.nonfinite != 1:
    error(f"one NaN: nonfinite {st.nonfinite}")
here = D.field_locate(x, "nonfinite")
if here != (cell if rank == who else None):
    error(f"field_locate: {here}, the NaN is at {cell} on rank {who + 1}")
try:
    D.psy.run_health([x, x], ["a", "b"], masks=[md, None])
    error("run_health did not raise on a NaN")
except D.DlesmError as e:
    if "field a" not in str(e) or f"(i, j) = ({cell[0]}, {cell[1]}) on rank {who + 1}" not in str(e):
        error(f"run_health message: {e}")

if L.dlesm_wait_timed_out(0):
    error("a device-side wait gave up")
t = torch.tensor([errors])
dist.all_reduce(t)
dist.barrier()
print(f"rank {rank}: tile {it.nx}x{it.ny} of {NX}x{NY}, errors {errors} (all ranks {int(t.item())})", flush=True)
D.parallel_finalise()
dist.destroy_process_group()
sys.exit(1 if int(t.item()) else 0)
