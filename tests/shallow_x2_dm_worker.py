"""One rank of the N-process test of the two-steps-per-call distributed shallow-water entries (dlesm_shallow_step_x2_dm,
dlesm_shallow_step_smooth_x2_dm; tests/test_a_shallow_x2_dm_ranks_gpu.py).  The ranks are separate processes sharing device 0
in mailbox mode: the decomposition (halo_width = 2) and the depth-2 message tables are the product's own, the blobs travel
through a gloo group, no RCCL.  Unlike loop-back, tiles here have sides WITHOUT a neighbour next to grown sides: the fixed NE
boundary ring of the undivided domain meets a computed ring at sub-domain corners.

Check: N calls of each form against the oracle's 2N steps on the UNDIVIDED domain -- every internal cell and every depth-2
halo cell of the newest level that lies inside the global domain (its boundary ring included), bit for bit; the filtered
form's filtered level likewise.

    RANK=r WORLD_SIZE=n MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/shallow_x2_dm_worker.py NX NY NDX NDY CALLS
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NX, NY, NDX, NDY, CALLS = (int(a) for a in sys.argv[1:6])
ALPHA = 0.1
SEED = 20261015
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

dist.init_process_group("gloo", rank=rank, world_size=world)
import dl_esm_inf_amd as D  # noqa: E402
import oracle_lib as O  # noqa: E402
import sw_numpy  # noqa: E402

torch.cuda.set_device(0)
L = D._cabi.lib()
L.dlesm_set_tuning(b"dm_wait_seconds", 30)         # a protocol error must end in words, not in a hung box
D.parallel_init(rank, world, transport="mailbox")
os.environ["DL_ESM_ALIGNMENT"] = "64"
g = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
g.decompose(NX, NY, ndomains=world, ndomainx=NDX, ndomainy=NDY, halo_width=2)
D.grid_init(g, 1.0, 1.0)
NAMES = ["u", "v", "p", "uold", "vold", "pold", "unew", "vnew", "pnew", "unew2", "vnew2", "pnew2"]
pts = {"u": D.GO_U_POINTS, "v": D.GO_V_POINTS, "p": D.GO_T_POINTS}
F = {n: D.r2d_field(g, pts[n[0]]) for n in NAMES}
it = F["p"].internal
sub = g.subdomain
prm = D.psy.shallow_params(1.0e5, 1.0e5, 90.0)

# The undivided domain, padded by one cell beyond its fixed boundary ring: global cell gi (0 and NX+1 = the ring) sits at
# index gi + 1, so a tile's 2-deep halos on a side without a neighbour map to the ring and to the padding.  Every time level
# carries the same boundary ring (what the single-domain entries ask for: the ring is fixed).
GLD, GNY = NX + 4, NY + 4
GBOX = (3, NX + 2, 3, NY + 2)             # the global internal region, 1-based, in the padded arrays
ox = sub.glob.xstart - it.xstart + 2      # padded index of local (0-based) column 0
oy = sub.glob.ystart - it.ystart + 2


def level(seed, add, ring_of=None):
    f = O.hash_field(seed, GNY, GLD, 0, 0, 1, GLD, 1, GNY) * 0.01 + add
    if ring_of is not None:
        inner = f[2:NY + 2, 2:NX + 2].copy()
        f = ring_of.copy()
        f[2:NY + 2, 2:NX + 2] = inner
    return f


G = {}
for k, n in enumerate(("u", "v", "p")):
    add = 1.0 if n == "p" else -0.005
    G[n] = level(SEED + k, add)
    G[n + "old"] = level(SEED + 100 + k, add, ring_of=G[n])


def local(glob):
    """this tile's window of a padded global array (cells beyond it: 0)"""
    out = np.zeros((g.ny, g.nx))
    y0, x0 = max(0, -oy), max(0, -ox)
    y1, x1 = min(g.ny, GNY - oy), min(g.nx, GLD - ox)
    out[y0:y1, x0:x1] = glob[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return out


def compare(fld, want, what):
    """internal cells and depth-2 halos that lie inside the global domain (its ring included)"""
    got = fld.get_data()
    bad = 0
    for j in range(it.ystart - 3, it.ystop + 2):
        gj = j + oy
        if gj < 1 or gj > NY + 2:
            continue
        xs = [i for i in range(it.xstart - 3, it.xstop + 2) if 1 <= i + ox <= NX + 2]
        row_got = got[j, xs[0]:xs[-1] + 1]
        row_want = want[gj, xs[0] + ox:xs[-1] + ox + 1]
        bad += int(np.count_nonzero(row_got != row_want))
    if bad:
        print(f"ERROR rank {rank}: {what}: {bad} cells differ from the undivided oracle", flush=True)
    return bad


def upload():
    for n in ("u", "v", "p"):
        F[n].set_data(local(G[n]))
        F[n + "old"].set_data(local(G[n + "old"]))
        for tag in ("new", "new2"):
            F[n + tag].set_data(local(G[n]))        # the fixed ring; the rest is overwritten


errors = 0
# ---- plain form: CALLS calls with the rotation (cur, old, new1, new2) <- (new2, new1, old, cur), against 2 x CALLS steps
upload()
cur = [G[n].copy() for n in ("u", "v", "p")]
old = [G[n + "old"].copy() for n in ("u", "v", "p")]
for _ in range(2 * CALLS):
    new = [c.copy() for c in cur]                   # (the ring of the new level = the fixed ring)
    O.sw_step(prm, GLD, GBOX, *cur, *old, *new)
    cur, old = new, cur
cf = [F[n] for n in ("u", "v", "p")]
of = [F[n] for n in ("uold", "vold", "pold")]
n1 = [F[n] for n in ("unew", "vnew", "pnew")]
n2 = [F[n] for n in ("unew2", "vnew2", "pnew2")]
s = torch.cuda.Stream()
for k in range(CALLS):
    D.psy.invoke_shallow_step_x2_dm(prm, *cf, *of, *n1, *n2, stream=s)
    cf, of, n1, n2 = n2, n1, of, cf
    if k == CALLS // 2:                              # ranks skewed against each other
        s.synchronize()
        import time
        time.sleep(0.03 * rank)
s.synchronize()
for k, n in enumerate("uvp"):
    errors += compare(cf[k], cur[k], f"plain form, newest level {n}")

# ---- filtered form: CALLS calls, ping-pong (cur, old) <-> (unew2.., uold2..), against 2 x CALLS filtered steps
upload()
cur = [G[n].copy() for n in ("u", "v", "p")]
old = [G[n + "old"].copy() for n in ("u", "v", "p")]
for _ in range(2 * CALLS):
    new = [c.copy() for c in cur]
    O.sw_step(prm, GLD, GBOX, *cur, *old, *new)
    for c, nw, o in zip(cur, new, old):
        sw_numpy.time_smooth_numpy(ALPHA, GBOX, c, nw, o)     # old <- the filtered current level
    cur = new
A = [F[n] for n in ("u", "v", "p", "uold", "vold", "pold")]
B = [F[n] for n in ("unew2", "vnew2", "pnew2", "unew", "vnew", "pnew")]
for k in range(CALLS):
    D.psy.invoke_shallow_step_smooth_x2_dm(prm, ALPHA, *A, *B, stream=s)
    A, B = B, A
s.synchronize()
for k, n in enumerate("uvp"):
    errors += compare(A[k], cur[k], f"filtered form, newest level {n}")
    errors += compare(A[3 + k], old[k], f"filtered form, filtered level {n}")

if L.dlesm_ipc_open_retries():
    print(f"ERROR rank {rank}: hipIpcOpenMemHandle had to be retried {L.dlesm_ipc_open_retries()} time(s)", flush=True)
    errors += 1
if L.dlesm_wait_timed_out(0):
    print(f"ERROR rank {rank}: a device-side wait gave up", flush=True)
    errors += 1
t = torch.tensor([errors])
dist.all_reduce(t)
dist.barrier()
print(f"rank {rank}: tile {it.nx}x{it.ny} of {NX}x{NY}, {2 * CALLS} steps per form, errors {errors} (all ranks {int(t.item())})",
      flush=True)
D.parallel_finalise()
dist.destroy_process_group()
sys.exit(1 if int(t.item()) else 0)
