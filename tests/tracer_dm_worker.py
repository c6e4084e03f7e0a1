"""One rank of the N-process test of tracer transport on a decomposed grid (dlesm_tracer_step_dm through
psy.invoke_tracer_step_dm; tests/test_a_tracer_dm_ranks_gpu.py).  The ranks are separate processes sharing device 0 in mailbox
mode: the decomposition (halo_width = 1) and the message tables are the product's own, the blobs travel through a gloo group,
no RCCL.

One model: a tidal open channel with a current along it and an island across the tile boundaries, STEPS steps of
invoke_nemolite_step_dm + invoke_tracer_step_dm with two tracers (c = 1, and a dye in [0, 1]), every rank against the CPU loop
of tests/tracer_cases.py run on the UNDIVIDED domain.  Checked after every step: every internal cell and every depth-1 halo
cell, inside the global array, of the thirteen flow arrays and of both tracers, bit for bit.  grid_init's tmask is in local
array coordinates: each rank passes its window of the global mask, its ring included.

    RANK=r WORLD_SIZE=n MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/tracer_dm_worker.py NX NY NDX NDY STEPS
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NX, NY, NDX, NDY, STEPS = (int(a) for a in sys.argv[1:6])
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

dist.init_process_group("gloo", rank=rank, world_size=world)
import dl_esm_inf_amd as D  # noqa: E402
import open_bc_numpy as B  # noqa: E402
import tracer_cases as TC  # noqa: E402
import tracer_numpy as TN  # noqa: E402
from nemolite_boxes import INS, OUTS  # noqa: E402

torch.cuda.set_device(0)
L = D._cabi.lib()
L.dlesm_set_tuning(b"dm_wait_seconds", 30)         # a protocol error must end in words, not in a hung box
D.parallel_init(rank, world, transport="mailbox")

GNY, GLD = NY + 2, NX + 2                 # the undivided domain and its one-cell ring
GBOX = (2, NX + 1, 2, NY + 1)             # its internal region, 1-based
OMEGA, LAT = 7.292116e-5, 50.0

user = TC.channel_user_mask(NX, NY)
user[NY // 2 - 6:NY // 2 + 5, NX // 2 - 9:NX // 2 + 8] = 0          # an island across the tile boundaries
G = TC.uniform_grid(user, TC.CHANNEL_DXY, LAT)

os.environ["DL_ESM_ALIGNMENT"] = "64"
g = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
g.decompose(NX, NY, ndomains=world, ndomainx=NDX, ndomainy=NDY)
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


D.grid_init(g, TC.CHANNEL_DXY, TC.CHANNEL_DXY, tmask=local(user, shape=(it.ystop + 1, it.xstop + 1)))
g.gphiu, g.gphiv = np.full((g.ny, g.nx), LAT), np.full((g.ny, g.nx), LAT)
D.psy.coriolis(g, OMEGA)
torch.cuda.synchronize()

H = TC.channel_state(user, NX, NY)
c_in, c_out = TC.channel_tracers(user)
T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
pts = {"ssha": T, "sshn_t": T, "ht": T, "sshn_u": U, "ssha_u": U, "un": U, "ua": U, "hu": U,
       "sshn_v": V, "ssha_v": V, "vn": V, "va": V, "hv": V}
F = {}
for k in TC.STATE:
    F[k] = D.r2d_field(g, pts[k])
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
    j0, j1 = max(ys - 2, -oy), min(ye, GNY - 1 - oy)            # the box and its depth-1 halos, inside the global array
    i0, i1 = max(xs - 2, -ox), min(xe, GLD - 1 - ox)
    pairs = [(k, F[k], H[k]) for k in TC.STATE] + [("tracer %d" % n, Co[n], c_out[n]) for n in range(2)]
    for name, fld, glob in pairs:
        got = fld.get_data()[j0:j1 + 1, i0:i1 + 1]
        want = glob[j0 + oy:j1 + oy + 1, i0 + ox:i1 + ox + 1]
        if not TN.same(got, want):
            n = int(np.count_nonzero((got != want) & ~(np.isnan(got) & np.isnan(want))))
            print(f"ERROR rank {rank}: step {step}: {name}: {n} cells differ from the undivided domain", flush=True)
            bad += 1
    return bad


prm = D.psy.momentum_params(*TC.CHANNEL_PRM)
rdt = TC.CHANNEL_PRM[0]
errors = 0
s = torch.cuda.Stream()
for step in range(STEPS):
    ssh_bc = D.psy.tide_ssh(*TC.CHANNEL_TIDE, (step + 1) * rdt)
    D.psy.invoke_nemolite_step_dm(prm, *[F[k] for k in OUTS], *[F[k] for k in INS], ssh_bc=ssh_bc, stream=s)
    D.psy.invoke_tracer_step_dm(rdt, Co, Ci, *[F[k] for k in ("ssha", "un", "vn", "ht", "hu", "hv", "sshn_t", "sshn_u",
                                                               "sshn_v")], stream=s)
    TC.cpu_step(G, GBOX, H, B.tide(*TC.CHANNEL_TIDE, (step + 1) * rdt), c_in, c_out, TC.CHANNEL_PRM)
    s.synchronize()
    errors += compare(step)
    for a, b in TC.ROTATE:
        F[a], F[b] = F[b], F[a]
    TC.rotate(H)
    Ci, Co, c_in, c_out = Co, Ci, c_out, c_in
wet = user > 0
if not (np.ptp(c_in[1][wet]) > 0.5 and float(np.abs(H["vn"]).max()) > 0.0):
    print(f"ERROR rank {rank}: the model did not move", flush=True)
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
