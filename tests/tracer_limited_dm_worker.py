"""One rank of the N-process test of limited tracer transport on a decomposed grid, SCHEME = muscl (second order:
dlesm_tracer_step_muscl_dm through psy.invoke_tracer_step_muscl_dm) or hancock (time-centred: dlesm_tracer_step_hancock_dm
through psy.invoke_tracer_step_hancock_dm); tests/test_a_tracer_dm_ranks_gpu.py.  The ranks are separate processes sharing
device 0 in mailbox mode: the decomposition (halo_width = 2) and the depth-2 message tables are the product's own, the blobs
travel through a gloo group, no RCCL.

Tracer-only steps: the flow is fixed -- random velocities of both signs in x and y over the open channel's mask with an island
across the tile boundaries, cut from the undivided arrays, so every rank's flow arrays hold valid halos of any depth -- and
STEPS calls of the scheme's wrapper carry two tracers, every rank against tests/tracer_muscl_numpy.py or
tests/tracer_hancock_numpy.py run on the UNDIVIDED domain.  Checked after every step: every internal cell and every depth-2 halo
cell, inside the global array, of both tracers, bit for bit.  muscl runs at tracer_cases.RDT.  hancock runs at rdt = 3.0e6,
which puts more than a tenth of the faces of the undivided domain's wet cells at a Courant number in (0, 1) and more than a
tenth at 1 or above (asserted on the host), so the factor, its fall-back to the upwind value and w of the cell beyond a tile's
box -- built from the depth-1 halos of area_t, ht and sshn_t -- are all compared.  The mask keeps the undivided domain's ring
free of wet cells (DESIGN.md sections 6.11 and 6.12).  grid_init gives the grid's mask its one-cell ring only and replicates it
outwards; the entries want valid depth-2 halos, so each rank sets the grid's host mask to its window of the global mask before
the device mirror is made.

    RANK=r WORLD_SIZE=n MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/tracer_limited_dm_worker.py SCHEME NX NY NDX NDY STEPS
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SCHEME = sys.argv[1]
assert SCHEME in ("muscl", "hancock"), SCHEME
NX, NY, NDX, NDY, STEPS = (int(a) for a in sys.argv[2:7])
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

dist.init_process_group("gloo", rank=rank, world_size=world)
import dl_esm_inf_amd as D  # noqa: E402
import tracer_cases as TC  # noqa: E402
import tracer_hancock_numpy as TH  # noqa: E402
import tracer_muscl_numpy as TM  # noqa: E402
import tracer_numpy as TN  # noqa: E402
from nemolite_boxes import _host_inputs  # noqa: E402

torch.cuda.set_device(0)
L = D._cabi.lib()
L.dlesm_set_tuning(b"dm_wait_seconds", 30)         # a protocol error must end in words, not in a hung box
D.parallel_init(rank, world, transport="mailbox")

GNY, GLD = NY + 2, NX + 2                 # the undivided domain and its one-cell ring
GBOX = (2, NX + 1, 2, NY + 1)             # its internal region, 1-based
DXY = 1000.0
# the wrapper, its restatement on the host, rdt
INVOKE, HOST_STEP, RDT = {"muscl": (D.psy.invoke_tracer_step_muscl_dm, TM.tracer_step_muscl, TC.RDT),
                          "hancock": (D.psy.invoke_tracer_step_hancock_dm, TH.tracer_step_hancock, 3.0e6)}[SCHEME]

user = TC.channel_user_mask(NX, NY)
user[NY // 2 - 6:NY // 2 + 5, NX // 2 - 9:NX // 2 + 8] = 0          # an island across the tile boundaries
ring = np.concatenate([user[0], user[-1], user[:, 0], user[:, -1]])
assert not (ring > 0).any()

os.environ["DL_ESM_ALIGNMENT"] = "64"
g = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
g.decompose(NX, NY, ndomains=world, ndomainx=NDX, ndomainy=NDY, halo_width=2)
os.environ.pop("DL_ESM_ALIGNMENT", None)
it = g.subdomain.internal
ox = g.subdomain.glob.xstart - it.xstart + 1      # global index of local (0-based) column 0
oy = g.subdomain.glob.ystart - it.ystart + 1


def local(glob, fill=0.0, shape=None):
    """this tile's window of a global array, of the grid's extents or `shape` (cells beyond the global array: fill)"""
    ny, nx = shape or (g.ny, g.nx)
    out = np.full((ny, nx), fill, dtype=glob.dtype)
    y0, x0 = max(0, -oy), max(0, -ox)
    y1, x1 = min(ny, GNY - oy), min(nx, GLD - ox)
    out[y0:y1, x0:x1] = glob[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


D.grid_init(g, DXY, DXY, tmask=local(user, shape=(it.ystop + 1, it.xstop + 1)))
g.tmask = np.ascontiguousarray(local(user))        # valid depth-2 halos of the mask; nothing outside the global array is wet
torch.cuda.synchronize()

rng = np.random.default_rng(20261018)              # every rank draws the same undivided arrays
Hall = _host_inputs(rng, user.shape)
Hall["ssha"] = 0.1 * rng.normal(size=user.shape)
H = {k: Hall[k] for k in TC.FLOW}
area_t = np.full(user.shape, DXY * DXY)
if SCHEME == "hancock":
    mid, big = TH.face_shares(RDT, GBOX, user, area_t, *[H[k] for k in TC.FLOW])
    assert mid >= 0.10 and big >= 0.10, (mid, big)
c_in, c_out = TC.tracers(rng, user.shape, 2)
c_out = [c.copy() for c in c_in]                   # an open cell's boundary value sits in both buffers
T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
pts = {"ssha": T, "un": U, "vn": V, "ht": T, "hu": U, "hv": V, "sshn_t": T, "sshn_u": U, "sshn_v": V}
F = {}
for k, p in pts.items():
    F[k] = D.r2d_field(g, p)
    F[k].set_data(local(H[k]))


def tracer_fields(arrays):
    out = []
    for a in arrays:
        f = D.r2d_field(g, T)
        f.set_data(local(a))
        out.append(f)
    return out


Ci, Co = tracer_fields(c_in), tracer_fields(c_out)
xs, xe, ys, ye = it.xstart, it.xstop, it.ystart, it.ystop


def compare(step):
    bad = 0
    j0, j1 = max(ys - 3, -oy), min(ye + 1, GNY - 1 - oy)        # the box and its depth-2 halos, inside the global array
    i0, i1 = max(xs - 3, -ox), min(xe + 1, GLD - 1 - ox)
    for n in range(2):
        got = Co[n].get_data()[j0:j1 + 1, i0:i1 + 1]
        want = c_out[n][j0 + oy:j1 + oy + 1, i0 + ox:i1 + ox + 1]
        if not TN.same(got, want):
            m = int(np.count_nonzero((got != want) & ~(np.isnan(got) & np.isnan(want))))
            print(f"ERROR rank {rank}: step {step}: tracer {n}: {m} cells differ from the undivided domain", flush=True)
            bad += 1
    return bad


errors = 0
start = [c.copy() for c in c_in]
s = torch.cuda.Stream()
for step in range(STEPS):
    INVOKE(RDT, Co, Ci, *[F[k] for k in pts], stream=s)
    HOST_STEP(RDT, GBOX, user, area_t, *[H[k] for k in TC.FLOW], c_in, c_out)
    s.synchronize()
    errors += compare(step)
    Ci, Co, c_in, c_out = Co, Ci, c_out, c_in
wet = user > 0
if not (np.isfinite(c_in[0][wet]).all() and (c_in[0][wet] != start[0][wet]).mean() > 0.9):
    print(f"ERROR rank {rank}: the tracers did not move", flush=True)
    errors += 1

if L.dlesm_ipc_open_retries():
    print(f"ERROR rank {rank}: hipIpcOpenMemHandle had to be retried {L.dlesm_ipc_open_retries()} time(s)", flush=True)
    errors += 1
if L.dlesm_wait_timed_out(0):
    print(f"ERROR rank {rank}: a device-side wait gave up", flush=True)
    errors += 1
t = torch.tensor([errors])
dist.all_reduce(t)
dist.barrier()
print(f"rank {rank}: tile {it.nx}x{it.ny} of {NX}x{NY}, {STEPS} steps, errors {errors} (all ranks {int(t.item())})", flush=True)
D.parallel_finalise()
dist.destroy_process_group()
sys.exit(1 if int(t.item()) else 0)
