"""One rank of the N-process test of the particle migration (dlesm_migrate_f64 through psy.particle_migrate;
tests/test_a_particle_migrate_ranks_gpu.py).  The ranks are separate processes sharing device 0 in mailbox mode: the
decomposition and the message tables are the product's own, so the neighbours and the shifts are those psy.migrate_neighbours
derives from them.

One model: a closed basin with one gyre and an island across the tile boundaries (tests/particle_migrate_numpy.py), constant
metrics, the flow fields set from this rank's windows of the global arrays.  STEPS steps of psy.drifter_step(nsub = 1) followed
by psy.particle_migrate with a cap small enough to hold particles back; every rank runs the numpy World of ALL ranks beside it
and compares its own slots, payload and record with it after every step, bit for bit.  At the end every id must be in exactly
one slot over all ranks (a gloo all-gather), and then rank 1 is handed more arrivals than it has FREE slots: the wrapper must
raise there and nowhere else.

    RANK=r WORLD_SIZE=n MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/particle_migrate_worker.py NX NY NDX NDY STEPS
"""
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
import drifter_numpy as DN  # noqa: E402
import particle_migrate_numpy as M  # noqa: E402

torch.cuda.set_device(0)
L = D._cabi.lib()
L.dlesm_set_tuning(b"dm_wait_seconds", 30)         # a protocol error must end in words, not in a hung box
D.parallel_init(rank, world, transport="mailbox")

DXY, H, NSEEDS, NSLOTS, CAP = 1000.0, 400.0, 6000, 4096, 10
tm, _, _, gun, gvn = M.gyre(NX, NY)
flow = (tm, np.full(tm.shape, DXY), np.full(tm.shape, DXY), gun, gvn)

g = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
g.decompose(NX, NY, ndomainx=NDX, ndomainy=NDY)             # (ndomains would ask for the automatic tiling)
subs = g.decomp.subdomains
MESH = (g.decomp._info.nx, g.decomp._info.ny)
# every rank's tile in the World's terms: x_global = x_local + off, global = the (NY + 2) x (NX + 2) array, 1-based
tiles = []
for r in range(world):
    it, gl = subs[r].internal, subs[r].glob
    tiles.append(dict(box=(it.xstart, it.xstop, it.ystart, it.ystop), off=(gl.xstart - it.xstart + 1, gl.ystart - it.ystart + 1),
                      shape=(it.ystop + 1, it.xstop + 1)))
me = tiles[rank]
it = g.subdomain.internal
D.grid_init(g, DXY, DXY, tmask=M.window(tm, me))
mine = dict(me, shape=(g.ny, g.nx))
un, vn = D.r2d_field(g, D.GO_U_POINTS), D.r2d_field(g, D.GO_V_POINTS)
un.set_data(M.window(gun, mine, 0.0)), vn.set_data(M.window(gvn, mine, 0.0))
torch.cuda.synchronize()

rng = np.random.default_rng(2121)
x, y = 2.0 + NX * rng.random(NSEEDS), 2.0 + NY * rng.random(NSEEDS)
w = M.World(flow, tiles, MESH, nslots=NSLOTS, cap=CAP, x=x, y=y, npayload=2)
errors = 0


def complain(text):
    global errors
    errors += 1
    print(f"ERROR rank {rank}: {text}", flush=True)


nb, sx, sy = D.psy.migrate_neighbours(g)
if (nb, sx, sy) != tuple(list(v) for v in w.links[rank]):
    complain(f"neighbours and shifts {(nb, sx, sy)} differ from the World's {w.links[rank]}")

up = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
px, py, st, ids = up(w.px[rank]), up(w.py[rank]), up(w.st[rank]), up(w.ids[rank])
pay = [up(a) for a in w.payload[rank]]
s = torch.cuda.Stream()
moved = held = 0
for step in range(STEPS):
    D.psy.drifter_step(H, px, py, st, un, vn, nsub=1, stream=s)
    rec = D.psy.particle_migrate(px, py, st, ids, un, payload=pay, cap=CAP, stream=s)
    w.step(H)
    s.synchronize()
    want = (w.px[rank], w.py[rank], w.st[rank], w.ids[rank]) + tuple(w.payload[rank])
    for name, got, ref in zip(("px", "py", "status", "id", "payload 0", "payload 1"), (px, py, st, ids) + tuple(pay), want):
        if not DN.same(got.cpu().numpy().view(ref.dtype), ref):
            complain(f"step {step}: {name} differs from the numpy World")
    if rec.as16() != tuple(int(v) for v in w.counts[rank]):
        complain(f"step {step}: the record {rec} differs from the World's {w.counts[rank]}")
    moved += sum(rec.sent)
    held += sum(rec.held)

# every id exactly once, over all ranks
live = ids[st != M.FREE].cpu()
sizes = [torch.zeros(1, dtype=torch.int64) for _ in range(world)]
dist.all_gather(sizes, torch.tensor([live.numel()]))
parts = [torch.zeros(NSLOTS, dtype=torch.int64) for _ in range(world)]
padded = torch.zeros(NSLOTS, dtype=torch.int64)
padded[:live.numel()] = live
dist.all_gather(parts, padded)
everyone = np.sort(np.concatenate([p[:int(k)].numpy() for p, k in zip(parts, sizes)]))
if not np.array_equal(everyone, np.arange(NSEEDS)):
    complain(f"{len(everyone)} ids over all ranks, {len(np.unique(everyone))} different ones, {NSEEDS} seeded")
total = torch.tensor([moved, held])
dist.all_reduce(total)
if int(total[0]) < 100 or int(total[1]) == 0:
    complain(f"{int(total[0])} particles crossed and {int(total[1])} were held over all ranks: the run shows nothing")

# too few FREE slots: rank 0 sends three particles east, rank 1 has one FREE slot -- the wrapper raises there alone
if MESH[0] >= 2:
    n2 = 4
    b = tiles[rank]["box"]
    qx = torch.full((n2,), b[1] + 1.25, dtype=torch.float64, device="cuda")
    qy = torch.full((n2,), b[2] + 0.5, dtype=torch.float64, device="cuda")
    qs = torch.tensor([M.LEFT] * 3 + [M.ACTIVE] if rank == 0 else [M.ACTIVE] * 3 + [M.FREE], dtype=torch.int32, device="cuda")
    if rank > 0:
        qx.fill_(b[0] + 0.5)
    qi = torch.arange(n2, dtype=torch.int64, device="cuda") + 100 * rank
    try:
        rec = D.psy.particle_migrate(qx, qy, qs, qi, g, cap=8)
        if rank == 1:
            complain(f"no MigrateError although arrivals were dropped: {rec}")
        elif rank == 0 and (rec.sent[M.E], rec.nfree) != (3, 3):
            complain(f"rank 0's record after sending three east: {rec}")
    except D.MigrateError as e:
        if rank != 1 or e.counts.dropped != 2 or e.counts.arrived[M.W] != 1 or e.counts.nfree != 0:
            complain(f"MigrateError {e} with {getattr(e, 'counts', None)}")

if L.dlesm_ipc_open_retries():
    complain(f"hipIpcOpenMemHandle had to be retried {L.dlesm_ipc_open_retries()} time(s)")
if L.dlesm_wait_timed_out(0):
    complain("a device-side wait gave up")
t = torch.tensor([errors])
dist.all_reduce(t)
dist.barrier()
print(f"rank {rank}: tile {it.nx}x{it.ny} of {NX}x{NY}, {STEPS} steps, {moved} sent, {held} held, errors {errors} "
      f"(all ranks {int(t.item())})", flush=True)
D.parallel_finalise()
dist.destroy_process_group()
sys.exit(1 if int(t.item()) else 0)
