"""One rank of the N-process test of the Jacobi step with its residual on a decomposed grid (psy.invoke_jacobi5_residual;
tests/test_a_jacobi_residual_ranks_gpu.py).  The ranks are separate processes sharing device 0 in mailbox mode: the
decomposition (halo_width = 1) and the message tables are the product's own, the blobs travel through a gloo group, no RCCL.

A Laplace solve: pipelined distributed steps (invoke_jacobi5_dm_pipelined), every CHECK-th step the residual step with
norm "max", until max|out - in| <= TOL; every rank runs the oracle's loop on the UNDIVIDED domain next to it.  At every check:
the global max equals the undivided domain's bit for bit, the stopping decision is the same, and the rank's box and depth-1
halos (inside the global array) equal the undivided field -- the residual call leaves `out` exchanged.  Then one residual step
with norm "l2" against math.fsum on the undivided domain (1e-12), and dlesm_global_max_f64 on its own: a max in rank order, a
NaN on one rank gives NaN on all.

    RANK=r WORLD_SIZE=n MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/jacobi_residual_worker.py NX NY NDX NDY
"""
import ctypes as C
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NX, NY, NDX, NDY = (int(a) for a in sys.argv[1:5])
SEED, TOL, CHECK, MAX_STEPS = 20261016, 1e-2, 5, 4000
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

dist.init_process_group("gloo", rank=rank, world_size=world)
import dl_esm_inf_amd as D  # noqa: E402
import oracle_lib as O  # noqa: E402

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


def local(glob):
    """this tile's window of a global array (cells beyond the global array: 0)"""
    out = np.zeros((g.ny, g.nx))
    y0, x0 = max(0, -oy), max(0, -ox)
    y1, x1 = min(g.ny, GNY - oy), min(g.nx, GLD - ox)
    out[y0:y1, x0:x1] = glob[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


GH = np.random.default_rng(SEED).random((GNY, GLD))
x, y = D.r2d_field(g, D.GO_T_POINTS), D.r2d_field(g, D.GO_T_POINTS)
x.set_data(local(GH))
y.set_data(local(GH))
assert x.internal.box() == (it.xstart, it.xstop, it.ystart, it.ystop)
j0, j1 = max(it.ystart - 2, -oy), min(it.ystop, GNY - 1 - oy)      # the box and its depth-1 halos, inside the global array
i0, i1 = max(it.xstart - 2, -ox), min(it.xstop, GLD - 1 - ox)


def same_as_global(fld, H, what):
    got = fld.get_data()[j0:j1 + 1, i0:i1 + 1]
    want = H[j0 + oy:j1 + oy + 1, i0 + ox:i1 + ox + 1]
    if not np.array_equal(got, want):
        error(f"{what}: {int(np.count_nonzero(got != want))} cells of the box and its halos differ from the undivided domain")


src, dst = x, y
hs, hd = GH.copy(), GH.copy()
step, checks, stop = 0, 0, None
while step < MAX_STEPS:
    step += 1
    O.jacobi5(hs, hd, GLD, 2, NX + 1, 2, NY + 1)
    if step % CHECK:
        D.psy.invoke_jacobi5_dm_pipelined(dst, src)
    else:
        r = D.psy.invoke_jacobi5_residual(dst, src, "max")
        want = float(np.max(np.abs(hd - hs)[1:NY + 1, 1:NX + 1]))
        checks += 1
        if r != want:
            error(f"step {step}: global max {r!r}, undivided domain {want!r}")
        same_as_global(dst, hd, f"step {step}")
        if (r <= TOL) != (want <= TOL):
            error(f"step {step}: stopping decisions differ ({r!r}, {want!r})")
        if want <= TOL:
            stop = step
            break
    src, dst = dst, src
    hs, hd = hd, hs
if stop is None:
    error(f"no convergence to {TOL} in {MAX_STEPS} steps")

# one more step, its residual as the l2 norm
src, dst = dst, src
hs, hd = hd, hs
O.jacobi5(hs, hd, GLD, 2, NX + 1, 2, NY + 1)
r2 = D.psy.invoke_jacobi5_residual(dst, src, "l2")
dd = (hd - hs)[1:NY + 1, 1:NX + 1]
want2 = math.sqrt(math.fsum((dd * dd).ravel()))
if not abs(r2 - want2) <= 1e-12 * want2:
    error(f"l2 {r2!r}, undivided domain {want2!r}")
same_as_global(dst, hd, "after the l2 step")

# dlesm_global_max_f64 by itself
v = C.c_double(rank + 0.5)
D._cabi.check(L.dlesm_global_max_f64(C.byref(v)))
if v.value != world - 0.5:
    error(f"global max of rank + 0.5: {v.value}")
v = C.c_double(float("nan") if rank == world - 1 else float(rank))
D._cabi.check(L.dlesm_global_max_f64(C.byref(v)))
if not math.isnan(v.value):
    error(f"global max with a NaN on rank {world - 1}: {v.value}")
v = C.c_double(-math.inf if rank else 3.0)
D._cabi.check(L.dlesm_global_max_f64(C.byref(v)))
if v.value != 3.0:
    error(f"global max of 3 and -inf: {v.value}")

if L.dlesm_wait_timed_out(0):
    error("a device-side wait gave up")
t = torch.tensor([errors])
dist.all_reduce(t)
stops = [None] * world
dist.all_gather_object(stops, stop)
dist.barrier()
print(f"rank {rank}: tile {it.nx}x{it.ny} of {NX}x{NY}, stop at step {stop} after {checks} checks, stops of all ranks {stops}, "
      f"errors {errors} (all ranks {int(t.item())})", flush=True)
D.parallel_finalise()
dist.destroy_process_group()
sys.exit(1 if int(t.item()) else 0)
