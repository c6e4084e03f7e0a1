"""One rank of the N-process test of the coupled step on a decomposed grid (dlesm_nemolite_coupled_step_dm through
psy.invoke_nemolite_coupled_step_dm, and dlesm_halo_exchange_i32 through grid_mod.exchange_mask_halos;
tests/test_a_coupled_dm_ranks_gpu.py).  The ranks are separate processes sharing device 0 in mailbox mode: the decomposition
(halo_width = HW) and the message tables are the product's own, the blobs travel through a gloo group, no RCCL.

The model is tests/tracer_dm_worker.py's: a tidal open channel with a current along it and an island across the tile boundaries,
two tracers (c = 1, and a dye in [0, 1]).  STEPS steps of ONE call each, invoke_nemolite_coupled_step_dm with SCHEME, every rank
against the CPU loops run on the UNDIVIDED domain: tests/tracer_cases.py's step for the flow and tests/tracer_hancock_numpy.py
("hancock") or tests/tracer_numpy.py ("upwind") for the tracers.  Checked after every step: every internal cell and every halo
cell of depth HW, inside the global array, of the thirteen flow arrays and of both tracers, bit for bit.

The mask: grid_init gets the rank's window of the global mask (its one-cell ring included) and replicates that ring outwards;
exchange_mask_halos then fetches the halos from the neighbours, and g.tmask must equal the window of the global mask in every
halo cell inside the global array.  The mask keeps the undivided domain's ring free of wet cells.

    RANK=r WORLD_SIZE=n MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/coupled_dm_worker.py NX NY NDX NDY STEPS SCHEME HW
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NX, NY, NDX, NDY, STEPS = (int(a) for a in sys.argv[1:6])
SCHEME, HW = sys.argv[6], int(sys.argv[7])
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

dist.init_process_group("gloo", rank=rank, world_size=world)
import dl_esm_inf_amd as D  # noqa: E402
import open_bc_numpy as B  # noqa: E402
import tracer_cases as TC  # noqa: E402
import tracer_hancock_numpy as TH  # noqa: E402
import tracer_numpy as TN  # noqa: E402
from dl_esm_inf_amd import grid_mod  # noqa: E402
from nemolite_boxes import INS, OUTS  # noqa: E402

torch.cuda.set_device(0)
L = D._cabi.lib()
L.dlesm_set_tuning(b"dm_wait_seconds", 30)         # a protocol error must end in words, not in a hung box
D.parallel_init(rank, world, transport="mailbox")

GNY, GLD = NY + 2, NX + 2                 # the undivided domain and its one-cell ring
GBOX = (2, NX + 1, 2, NY + 1)             # its internal region, 1-based
OMEGA, LAT = 7.292116e-5, 50.0
CPU_TRACERS = {"hancock": TH.tracer_step_hancock, "upwind": TN.tracer_step}[SCHEME]

user = TC.channel_user_mask(NX, NY)
user[NY // 2 - 6:NY // 2 + 5, NX // 2 - 9:NX // 2 + 8] = 0          # an island across the tile boundaries
ring = np.concatenate([user[0], user[-1], user[:, 0], user[:, -1]])
assert not (ring > 0).any()
G = TC.uniform_grid(user, TC.CHANNEL_DXY, LAT)

os.environ["DL_ESM_ALIGNMENT"] = "64"
g = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
g.decompose(NX, NY, ndomains=world, ndomainx=NDX, ndomainy=NDY, halo_width=HW)
os.environ.pop("DL_ESM_ALIGNMENT", None)
it = g.subdomain.internal
ox = g.subdomain.glob.xstart - it.xstart + 1      # global index of local (0-based) column 0
oy = g.subdomain.glob.ystart - it.ystart + 1
xs, xe, ys, ye = it.xstart, it.xstop, it.ystart, it.ystop
# the box and its halos of depth HW, inside the global array (0-based, inclusive)
J0, J1 = max(ys - 1 - HW, -oy), min(ye - 1 + HW, GNY - 1 - oy)
I0, I1 = max(xs - 1 - HW, -ox), min(xe - 1 + HW, GLD - 1 - ox)


def local(glob, fill=0.0, shape=None):
    """this tile's window of a global array, of the grid's extents or `shape` (cells beyond the global array: fill)"""
    ny, nx = shape or (g.ny, g.nx)
    out = np.full((ny, nx), fill, dtype=glob.dtype)
    y0, x0 = max(0, -oy), max(0, -ox)
    y1, x1 = min(ny, GNY - oy), min(nx, GLD - ox)
    out[y0:y1, x0:x1] = glob[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


errors = 0
D.grid_init(g, TC.CHANNEL_DXY, TC.CHANNEL_DXY, tmask=local(user, shape=(it.ystop + 1, it.xstop + 1)))
grid_mod.exchange_mask_halos(g)
if not np.array_equal(g.tmask[J0:J1 + 1, I0:I1 + 1], user[J0 + oy:J1 + oy + 1, I0 + ox:I1 + ox + 1]):
    n = int(np.count_nonzero(g.tmask[J0:J1 + 1, I0:I1 + 1] != user[J0 + oy:J1 + oy + 1, I0 + ox:I1 + ox + 1]))
    print(f"ERROR rank {rank}: the mask differs from the global mask's window in {n} cells of the box and its halos", flush=True)
    errors += 1
if not np.array_equal(g.tmask_device.cpu().numpy(), g.tmask):
    print(f"ERROR rank {rank}: the mask's device mirror and the host mask differ", flush=True)
    errors += 1
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


def compare(step):
    bad = 0
    pairs = [(k, F[k], H[k]) for k in TC.STATE] + [("tracer %d" % n, Co[n], c_out[n]) for n in range(2)]
    for name, fld, glob in pairs:
        got = fld.get_data()[J0:J1 + 1, I0:I1 + 1]
        want = glob[J0 + oy:J1 + oy + 1, I0 + ox:I1 + ox + 1]
        if not TN.same(got, want):
            n = int(np.count_nonzero((got != want) & ~(np.isnan(got) & np.isnan(want))))
            print(f"ERROR rank {rank}: step {step}: {name}: {n} cells differ from the undivided domain", flush=True)
            bad += 1
    return bad


prm = D.psy.momentum_params(*TC.CHANNEL_PRM)
rdt = TC.CHANNEL_PRM[0]
s = torch.cuda.Stream()
for step in range(STEPS):
    ssh_bc = D.psy.tide_ssh(*TC.CHANNEL_TIDE, (step + 1) * rdt)
    D.psy.invoke_nemolite_coupled_step_dm(prm, SCHEME, Co, Ci, *[F[k] for k in OUTS], *[F[k] for k in INS], ssh_bc=ssh_bc,
                                          stream=s)
    TC.cpu_step(G, GBOX, H, B.tide(*TC.CHANNEL_TIDE, (step + 1) * rdt), [], [], TC.CHANNEL_PRM)      # the flow
    CPU_TRACERS(rdt, GBOX, G.tmask, G.area_t, *[H[k] for k in TC.FLOW], c_in, c_out)
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
