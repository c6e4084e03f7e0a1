"""One rank of the N-process test of the one-call NEMOLite2D-class step on a decomposed grid (dlesm_nemolite_step_dm through
psy.invoke_nemolite_step_dm; tests/test_a_nemolite_step_dm_ranks_gpu.py).  The ranks are separate processes sharing device 0 in
mailbox mode: the decomposition (halo_width = 1) and the message tables are the product's own, the blobs travel through a gloo
group, no RCCL.

Two models, STEPS steps each, every rank against the CPU restatements (the continuity oracle, momentum_numpy, open_bc_numpy,
in the order of test_gpu_nemolite_step.py::_time_loop) run on the UNDIVIDED domain:
- a closed basin with an island across the tile boundaries and a bump of the surface;
- an open channel (open first and last internal columns) with a tidal ssh_bc: only the ranks on the west and east edges hold
  open cells, so the ranks' open-boundary plans have lists of different lengths, some empty.
Checked after every step: every internal cell and every depth-1 halo cell of all thirteen arrays that lies inside the global
array, bit for bit.  grid_init's tmask is in local array coordinates: each rank passes its window of the global mask, its
ring included; the metrics and the latitude are windows of global arrays too.

    RANK=r WORLD_SIZE=n MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/nemolite_step_dm_worker.py NX NY NDX NDY STEPS
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NX, NY, NDX, NDY, STEPS = (int(a) for a in sys.argv[1:6])
SEED = 20261015
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

dist.init_process_group("gloo", rank=rank, world_size=world)
import dl_esm_inf_amd as D  # noqa: E402
import momentum_numpy as M  # noqa: E402
import open_bc_numpy as B  # noqa: E402
import oracle_lib as O  # noqa: E402

torch.cuda.set_device(0)
L = D._cabi.lib()
L.dlesm_set_tuning(b"dm_wait_seconds", 30)         # a protocol error must end in words, not in a hung box
D.parallel_init(rank, world, transport="mailbox")

PRM = (20.0, 0.00015, 50.0, 9.80665)
METRICS = ("dx_t", "dy_t", "dx_u", "dy_u", "dx_v", "dy_v", "area_t", "area_u", "area_v")
INS = ("un", "vn", "ht", "hu", "hv", "sshn_t", "sshn_u", "sshn_v")
OUTS = ("ssha", "ssha_u", "ssha_v", "ua", "va")
MOM = ("un", "vn", "ht", "sshn_t", "hu", "sshn_u", "hv", "sshn_v", "ssha_u", "ssha_v")
NAMES = INS + OUTS
GNY, GLD = NY + 2, NX + 2                 # the undivided domain and its one-cell ring
GBOX = (2, NX + 1, 2, NY + 1)             # its internal region, 1-based
rng = np.random.default_rng(SEED)
GM = {}
for name in METRICS:
    a = 900.0 + 200.0 * rng.random((GNY, GLD))
    GM[name] = a * 1000.0 if name.startswith("area") else a
GPHIU = 40.0 + 20.0 * rng.random((GNY, GLD))
GPHIV = 40.0 + 20.0 * rng.random((GNY, GLD))
OMEGA = 7.292116e-5


def run_model(user, amp, bump):
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

    # (the grid's extents exist after grid_init: the mask covers local rows and columns up to the ring, 1-based ystop+1)
    D.grid_init(g, 1000.0, 1000.0, tmask=local(user, shape=(it.ystop + 1, it.xstop + 1)))
    for name in METRICS:
        getattr(g, name + "_device").copy_(torch.from_numpy(local(GM[name], 1.0)))
    g.gphiu, g.gphiv = local(GPHIU, 45.0), local(GPHIV, 45.0)
    D.psy.coriolis(g, OMEGA)
    torch.cuda.synchronize()
    G = M.SimpleNamespace(tmask=user, **GM, fcor_u=(2.0 * OMEGA) * np.sin(GPHIU * (math.pi / 180.0)),
                          fcor_v=(2.0 * OMEGA) * np.sin(GPHIV * (math.pi / 180.0)))
    H = {k: np.zeros((GNY, GLD)) for k in NAMES}
    for k in ("ht", "hu", "hv"):
        H[k][:] = 10.0
    if bump:
        jj, ii = np.mgrid[0:GNY, 0:GLD]
        H["sshn_t"][:] = 0.01 * np.exp(-((ii - 0.6 * NX) ** 2 + (jj - 0.5 * NY) ** 2) / (2 * (NX / 6.0) ** 2))
    T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
    pts = {"ssha": T, "sshn_t": T, "ht": T, "sshn_u": U, "ssha_u": U, "un": U, "ua": U, "hu": U,
           "sshn_v": V, "ssha_v": V, "vn": V, "va": V, "hv": V}
    F = {}
    for k in NAMES:
        F[k] = D.r2d_field(g, pts[k])
        F[k].set_data(local(H[k]))
    assert F["ssha"].internal.box() == F["ua"].internal.box() == F["va"].internal.box()
    xs, xe, ys, ye = it.xstart, it.xstop, it.ystart, it.ystop

    def compare(step):
        bad = 0
        j0, j1 = max(ys - 2, -oy), min(ye, GNY - 1 - oy)            # the box and its depth-1 halos, inside the global array
        i0, i1 = max(xs - 2, -ox), min(xe, GLD - 1 - ox)
        for k in NAMES:
            got = F[k].get_data()[j0:j1 + 1, i0:i1 + 1]
            want = H[k][j0 + oy:j1 + oy + 1, i0 + ox:i1 + ox + 1]
            if not M.same(got, want):
                n = int(np.count_nonzero((got != want) & ~(np.isnan(got) & np.isnan(want))))
                print(f"ERROR rank {rank}: step {step}: {k}: {n} cells differ from the undivided domain", flush=True)
                bad += 1
        return bad

    prm, hp = D.psy.momentum_params(*PRM), M.params(*PRM)
    rdt, omega = PRM[0], 2.0 * math.pi / (12.0 * 3600.0)
    nt = 0 if amp is None else D.psy.open_boundary(g).nt
    errors = 0
    s = torch.cuda.Stream()
    for step in range(STEPS):
        ssh_bc = None if amp is None else D.psy.tide_ssh(amp, omega, (step + 1) * rdt)
        D.psy.invoke_nemolite_step_dm(prm, *[F[k] for k in OUTS], *[F[k] for k in INS], ssh_bc=ssh_bc, stream=s)
        O.continuity_slabs(rdt, GLD, GBOX, H["sshn_t"], H["sshn_u"], H["sshn_v"], H["hu"], H["hv"], H["un"], H["vn"],
                           G.area_t, H["ssha"])
        if amp is not None:
            B.bc_ssh(GBOX, G.tmask, B.tide(amp, omega, (step + 1) * rdt), H["ssha"])
        M.next_sshu(GBOX, G.tmask, G.area_t, G.area_u, H["ssha"], H["ssha_u"])
        M.next_sshv(GBOX, G.tmask, G.area_t, G.area_v, H["ssha"], H["ssha_v"])
        M.momentum(hp, G, GBOX, GBOX, *[H[k] for k in MOM], H["ua"], H["va"])
        if amp is not None:
            B.flather_u(hp, GBOX, G.tmask, H["hu"], H["sshn_u"], H["sshn_t"], H["ua"])
            B.flather_v(hp, GBOX, G.tmask, H["hv"], H["sshn_v"], H["sshn_t"], H["va"])
        s.synchronize()
        errors += compare(step)
        if step == STEPS // 2:                         # ranks skewed against each other
            import time
            time.sleep(0.03 * rank)
        for a, b in (("un", "ua"), ("vn", "va"), ("sshn_t", "ssha"), ("sshn_u", "ssha_u"), ("sshn_v", "ssha_v")):
            F[a], F[b] = F[b], F[a]
            H[a], H[b] = H[b], H[a]
    moved = float(np.abs(H["un"]).max())
    if not moved > 0.0:
        print(f"ERROR rank {rank}: the model did not move", flush=True)
        errors += 1
    return errors, nt, it


# closed basin: land ring, an island across the middle of the domain (so across tile boundaries), a bump
basin = np.ones((GNY, GLD), dtype=np.int32)
basin[0, :] = basin[-1, :] = 0
basin[:, 0] = basin[:, -1] = 0
basin[NY // 2 - 6:NY // 2 + 5, NX // 2 - 9:NX // 2 + 8] = 0
e1, _, it = run_model(basin, None, True)
# open channel: open first and last internal columns, land rows north and south, a tide of period 12 h
chan = np.ones((GNY, GLD), dtype=np.int32)
chan[:, 0] = chan[:, -1] = 0
chan[:, 1] = chan[:, NX] = -1
chan[:2, :] = 0
chan[-2:, :] = 0
e2, nt, _ = run_model(chan, 0.1, False)
errors = e1 + e2

if L.dlesm_ipc_open_retries():
    print(f"ERROR rank {rank}: hipIpcOpenMemHandle had to be retried {L.dlesm_ipc_open_retries()} time(s)", flush=True)
    errors += 1
if L.dlesm_wait_timed_out(0):
    print(f"ERROR rank {rank}: a device-side wait gave up", flush=True)
    errors += 1
t = torch.tensor([errors])
dist.all_reduce(t)
counts = [None] * world
dist.all_gather_object(counts, nt)
dist.barrier()
print(f"rank {rank}: tile {it.nx}x{it.ny} of {NX}x{NY}, {STEPS} steps per model, open T cells per rank {counts}, "
      f"errors {errors} (all ranks {int(t.item())})", flush=True)
D.parallel_finalise()
dist.destroy_process_group()
sys.exit(1 if int(t.item()) else 0)
