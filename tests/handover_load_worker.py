"""The DEVICE-SIDE HAND-OVERS of the distributed steps, run LONG and checked WORD BY WORD, while
tests/handover_load.py competes for the CUs, the L2s and the fabric from a process of its own
(tests/test_a_handover_load_gpu.py starts both).  Modelled on tests/peer_two_ranks_worker.py.

    python tests/handover_load_worker.py loopback [--tiles 37x29,300x41,8x3,2048x2048] [--tune KEY=INT ...]
    RANK=r WORLD_SIZE=n MASTER_ADDR=.. MASTER_PORT=.. python tests/handover_load_worker.py ranks NXxNY:ALIGN[,...] MODE

Every form runs two passes from the same initial fields:
  pass A  N steps enqueued on one non-default stream with NOTHING between them (no host synchronisation, no copy, no other
          launch), one join, one synchronise; the newest level against N oracle steps, bit for bit, every internal word and
          every halo word the form defines.  These schemes carry every perturbation forward, so equal final bits mean that
          every operand of every step was the right one.
  pass B  the same steps with a device copy of the output into a history slab behind each step (same stream); every step's
          internal region is compared at the end: names the first wrong step.
The fields ping-pong (the output of step n is the input of step n + 1), the small tiles stay inside one XCD's L2, and every
halo line and mailbox half is rewritten two steps after it was read: a reader that misses an invalidate or a write-back sees
the value of step n - 1 or n - 2.  That only shows where those values differ, so the oracle's history is checked first:
the number of handed-over words whose value at step n equals their value at n - 1 or n - 2 must be ZERO for every n.

Prints `WINDOW <form> <pass> <t0> <t1>` (time.monotonic_ns() just before the first enqueue and just after the final
synchronise), `FORM <form> differ A=<words> B=<words> first_bad_step=<n>` and one `ERROR ...` line per failure."""
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

MODE = sys.argv[1]
SEED = 20261020
# internal size -> (alignment, steps): the smallest shapes at which these hand-overs can still go wrong.  The step counts are
# what a pass window needs to hold three launches of the load (a mailbox step of a small tile takes 8 us, of 2048^2 18 us, and
# beside the 2048^2 sweeps a launch of the load takes twice as long), within what the zero-unchanged-words condition allows: on 8x3 the periodic Jacobi field is flat to the last bit
# after 200 steps, the 3x3-weighted one after 143.
TILES = {"37x29": (None, 600),       # odd pitch: halo cells share lines with swept cells (section 8.1 row 5)
         "300x41": (64, 600),
         "8x3": (None, 160),         # frame-only launch, no interior
         "2048x2048": (64, 120)}      # many frame workgroups, spread over all XCDs (the Jacobi forms and the exchange only)
S9_STEPS = {"8x3": 120}
NEMO_STEPS = 300                     # (the restatement of the momentum update on the host is the slow part)
BIG = 1 << 20                        # tiles above this many cells run the one-field forms only
RANK_STEPS = {"jacobi": 400, "shallow": 200}
TUNING_DEFAULTS = {"dm_skip_parts": 0, "sw_x2_dm_overlap": 0, "j5_dm_chain": 1, "dm_peer_join_fused": 1, "dm_wait_seconds": 600, "dm_acquire": 1,
                   "mailbox_fences": 1}

if MODE == "ranks":
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
else:
    rank, world = 0, 1

import torch  # noqa: E402

if MODE == "ranks":
    import torch.distributed as dist  # noqa: E402
    dist.init_process_group("gloo", rank=rank, world_size=world)
import dl_esm_inf_amd as D  # noqa: E402
import oracle_lib as O  # noqa: E402

torch.cuda.set_device(0)
L = D._cabi.lib()
touched = set()


def tune(key, value):
    """dlesm_set_tuning keeps an unknown key without reading it: a misspelt or retired key would leave a form running in
    its default configuration under a label that says otherwise, so the key's class is asked for first"""
    if L.dlesm_tuning_class(key.encode()) < 0:
        raise SystemExit(f"ERROR rank {rank}: the library has no tuning key {key!r}")
    touched.add(key)
    L.dlesm_set_tuning(key.encode(), value)


tune("dm_wait_seconds", 30)          # a protocol error must end in words, not in a hung box
errors = 0
nforms = 0


def error(msg):
    global errors
    errors += 1
    print(f"ERROR rank {rank}: {msg}", flush=True)


def bits(t):
    return t.view(torch.int64)


def frame_of(a, x0, x1, y0, y1, depth=1):
    """the words a depth-`depth` exchange hands over: the outermost rows and columns of the (0-based, inclusive) box of `a`"""
    parts = []
    for d in range(depth):
        parts += [a[y0 + d, x0:x1 + 1], a[y1 - d, x0:x1 + 1], a[y0:y1 + 1, x0 + d], a[y0:y1 + 1, x1 - d]]
    return np.concatenate(parts)


def assert_every_handed_word_changes(frames, what):
    """frames[n] = the handed-over words of time level n (one array per field)"""
    same = 0
    for n in range(1, len(frames)):
        for back in (1, 2):
            if n - back >= 0:
                for new, old in zip(frames[n], frames[n - back]):
                    same += int(np.count_nonzero(new == old))
    if same:
        error(f"{what}: {same} handed-over words keep their value over one or two steps: a stale read of them would not show")


class Scheme:
    """one time-stepping scheme on one set of device fields, with the oracle's history of it.  record(level) takes the
    tuple of FULL host arrays of the next level, as the buffers that hold it must look after that many steps and a join:
    its handed-over words stay on the host (frames), the whole level goes to the device (history: every level for pass B,
    the last one for pass A)"""
    box0 = None            # 0-based inclusive internal box
    depth = 1              # of the exchange

    def record(self, level):
        if not hasattr(self, "frames"):
            self.frames, self.hist_dev = [], []
            self.level0 = tuple(a.copy() for a in level)
        else:
            one = len(level) == 1 and level[0].flags["C_CONTIGUOUS"]
            self.hist_dev.append(torch.from_numpy(level[0][None] if one else np.stack(level)).cuda())
        self.frames.append(tuple(frame_of(a, *self.box0, min(self.depth, self.box0[1] - self.box0[0] + 1, self.box0[3] - self.box0[2] + 1)) for a in level))

    def reset(self, s): ...
    def step(self, k, form, s): ...          # enqueue step k (0-based); returns the tensors that hold level k + 1
    def join(self, s): ...
    def final_region(self): ...              # boolean host mask of the words the final comparison covers

    def run(self, label, form, nsteps, setup=()):
        """both passes of one form; setup = ((tuning key, value), ...) for its duration"""
        global nforms
        nforms += 1
        for k, v in setup:
            tune(k, v)
        s = torch.cuda.Stream()
        y0, y1, x0, x1 = self.box0[2], self.box0[3], self.box0[0], self.box0[1]
        nf = len(self.level0)
        assert nsteps == len(self.frames) - 1, "the final comparison is with the LAST recorded level"
        bad = {}
        first_bad = -1
        for which in ("A", "B"):
            if which == "B":
                shape = self.level0[0].shape
                hist = torch.empty((nsteps, nf) + shape, dtype=torch.float64, device="cuda")
            self.reset(s)
            torch.cuda.synchronize()
            if MODE == "ranks":
                dist.barrier()
            t0 = time.monotonic_ns()
            if which == "A":
                for k in range(nsteps):
                    out = self.step(k, form, s)
            else:
                with torch.cuda.stream(s):
                    for k in range(nsteps):
                        out = self.step(k, form, s)
                        for f, o in enumerate(out):
                            hist[k, f].copy_(o, non_blocking=True)
            self.join(s)
            s.synchronize()
            t1 = time.monotonic_ns()
            print(f"WINDOW {label} {which} {t0} {t1}", flush=True)
            if which == "A":
                mask = self.final_region()
                n = 0
                for o, want in zip(out, self.device_history()[-1].cpu().numpy()):
                    n += int(np.count_nonzero((o.cpu().numpy().view(np.int64) != want.view(np.int64)) & mask))
                bad["A"] = n
            else:
                want = self.device_history()
                diff = (bits(hist)[:, :, y0:y1 + 1, x0:x1 + 1] != bits(want)[:, :, y0:y1 + 1, x0:x1 + 1]).flatten(1).sum(1)
                bad["B"] = int(diff.sum().item())
                if bad["B"]:
                    first_bad = int(torch.nonzero(diff)[0].item()) + 1
                del hist
        for k, _ in setup:
            tune(k, TUNING_DEFAULTS[k])
        print(f"FORM {label} differ A={bad['A']} B={bad['B']} first_bad_step={first_bad}", flush=True)
        if bad["A"]:
            error(f"{label}: pass A (undisturbed): {bad['A']} words of the newest level differ from {nsteps} oracle steps")
        if bad["B"]:
            error(f"{label}: pass B (located): {bad['B']} internal words differ, the first at step {first_bad}")

    _dev = None

    def device_history(self):
        if self._dev is None:
            self._dev = torch.stack(self.hist_dev)
            self.hist_dev = [None] * len(self.hist_dev)
        return self._dev


# ======================================================================================================= loop-back mode
def make_grid(nx, ny, alignment, hw=1):
    if alignment is None:
        os.environ.pop("DL_ESM_ALIGNMENT", None)
    else:
        os.environ["DL_ESM_ALIGNMENT"] = str(alignment)
    g = D.grid_type(D.GO_ARAKAWA_C, (1, 1, 2), D.GO_OFFSET_NE)
    g.decompose(nx, ny, halo_width=hw) if hw != 1 else g.decompose(nx, ny)
    D.grid_init(g, 1.0, 1.0)
    os.environ.pop("DL_ESM_ALIGNMENT", None)
    return g


EX_MASKS = [((1, 2, 3, 4), True), ((1, 2, 3, 4), False), ((1,), False), ((2, 4), True), ((), False), ((1, 2, 3), False),
            ((1, 4), False)]


class LoopJacobi(Scheme):
    """ping-pong of one T field; forms: joined / pipelined (dlesm_jacobi5_step_dm[_pipelined]), stencil9
    (dlesm_stencil9_step_dm, eight directions), exchange (plain sweep + dlesm_halo_exchange_f64 with a mask that changes
    from step to step: what is not exchanged in a step stays as it was, in the oracle too)"""

    def __init__(self, g, t, oc, nsteps, kind):
        self.g, self.kind = g, kind
        self.x, self.y = D.r2d_field(g, D.GO_T_POINTS), D.r2d_field(g, D.GO_T_POINTS)
        it = self.it = self.x.internal
        self.box0 = (it.xstart - 1, it.xstop - 1, it.ystart - 1, it.ystop - 1)
        self.coef = np.random.default_rng(9).random(9) + 0.2
        self.coef /= self.coef.sum()                      # positive weights that sum to one (to rounding): the field stays O(1)
        self.cp = self.coef.ctypes.data_as(C.POINTER(C.c_double))
        h0 = O.hash_field(SEED + 31, g.ny, g.nx, 0, 0, 1, g.nx, 1, g.ny)
        assert O.exchange_all([h0], [g.nx], [oc]) == 0
        self.init = torch.from_numpy(h0).cuda()
        hx, hy = h0.copy(), h0.copy()
        self.record((h0,))
        for k in range(nsteps):
            if kind == "stencil9":
                O.stencil9(hx, hy, self.coef, g.nx, *it.box())
                assert O.exchange_all([hy], [g.nx], [oc]) == 0
            else:
                O.jacobi5(hx, hy, g.nx, *it.box())
                dirs, nodiag = EX_MASKS[k % len(EX_MASKS)] if kind == "exchange" else ((1, 2, 3, 4), True)
                assert O.exchange_dirs([hy], [g.nx], [oc], dirs, no_diagonals=nodiag) == 0
            hx, hy = hy, hx
            self.record((hx,))
        assert_every_handed_word_changes(self.frames, f"{kind} on {it.nx}x{it.ny}")
        self.plan = None

    def reset(self, s):
        with torch.cuda.stream(s):
            self.x.data.copy_(self.init)
            self.y.data.copy_(self.init)

    def step(self, k, form, s):
        g, it = self.g, self.it
        a, b = (self.x, self.y) if k % 2 == 0 else (self.y, self.x)
        sp = C.c_void_p(s.cuda_stream)
        if form == "stencil9":
            rc = L.dlesm_stencil9_step_dm(self.plan, a.device_ptr, b.device_ptr, self.cp, g.nx, g.ny, *it.box(), sp)
        elif form == "exchange":
            dirs, nodiag = EX_MASKS[k % len(EX_MASKS)]
            mask = sum(1 << (d - 1) for d in dirs) | (D._cabi.DIRS_NO_DIAGONALS if nodiag else 0)
            rc = L.dlesm_stencil5_f64(a.device_ptr, b.device_ptr, g.nx, g.ny, *it.box(), sp)
            rc = rc or L.dlesm_halo_exchange_f64(self.plan, b.device_ptr, mask, sp)
        else:
            fn = L.dlesm_jacobi5_step_dm if form == "joined" else L.dlesm_jacobi5_step_dm_pipelined
            rc = fn(self.plan, a.device_ptr, b.device_ptr, g.nx, g.ny, *it.box(), sp)
        D._cabi.check(rc)
        return (b.data,)

    def join(self, s):
        D._cabi.check(L.dlesm_halo_plan_join(self.plan, C.c_void_p(s.cuda_stream)))

    def final_region(self):
        return np.ones((self.g.ny, self.g.nx), dtype=bool)        # the whole buffer: what no exchange writes keeps its bits


class LoopShallow(Scheme):
    """leapfrog rotation of nine fields; forms: joined / pipelined (dlesm_shallow_step_dm[_pipelined])"""
    names = ["u", "v", "p", "uold", "vold", "pold", "unew", "vnew", "pnew"]

    def __init__(self, g, t, oc, nsteps):
        self.g = g
        pts = {"u": D.GO_U_POINTS, "v": D.GO_V_POINTS, "p": D.GO_T_POINTS}
        self.F = {n: D.r2d_field(g, pts[n[0]]) for n in self.names}
        it = self.it = self.F["p"].internal
        self.box0 = (it.xstart - 1, it.xstop - 1, it.ystart - 1, it.ystop - 1)
        H = {}
        for k, n in enumerate(self.names):
            if k < 6:
                h = O.hash_field(SEED + 200 + k, g.ny, g.nx, 0, 0, 1, g.nx, 1, g.ny)
                h *= 0.01
                h += 1.0 if n[0] == "p" else -0.005
                assert O.exchange_all([h], [g.nx], [oc]) == 0
            else:
                h = np.full((g.ny, g.nx), 9.0)
            H[n] = h
        self.init = {n: torch.from_numpy(H[n]).cuda() for n in self.names}
        self.prm = D.psy.shallow_params(1.0e5, 1.0e5, 20.0)
        op = O.SwParams(self.prm.fsdx, self.prm.fsdy, self.prm.tdts8, self.prm.tdtsdx, self.prm.tdtsdy)
        scratch = [np.zeros((g.ny, g.nx)) for _ in range(4)]
        cur, old, new = self.names[:3], self.names[3:6], self.names[6:]
        self.record(tuple(H[n] for n in cur))
        for _ in range(nsteps):
            O.lib().orc_sw_step(C.byref(op), g.nx, *it.box(), *[H[n] for n in cur + old], *scratch, *[H[n] for n in new])
            for n in new:
                assert O.exchange_all([H[n]], [g.nx], [oc]) == 0
            cur, old, new = new, cur, old
            self.record(tuple(H[n] for n in cur))
        assert np.isfinite(H[cur[2]]).all()
        assert_every_handed_word_changes(self.frames, f"shallow water on {it.nx}x{it.ny}")

    def reset(self, s):
        with torch.cuda.stream(s):
            for n in self.names:
                self.F[n].data.copy_(self.init[n])

    def step(self, k, form, s):
        r = k % 3
        nm = self.names
        order = (nm[0:3], nm[3:6], nm[6:9]), (nm[6:9], nm[0:3], nm[3:6]), (nm[3:6], nm[6:9], nm[0:3])
        cur, old, new = order[r]
        fn = D.psy.invoke_shallow_step_dm if form == "joined" or (form == "alternate" and k % 2 == 0) \
            else D.psy.invoke_shallow_step_dm_pipelined
        fn(self.prm, *[self.F[n] for n in cur + old + new], stream=s)
        return tuple(self.F[n].data for n in new)

    def join(self, s):
        D.psy.halo_join(self.g, stream=s)

    def final_region(self):
        return np.ones((self.g.ny, self.g.nx), dtype=bool)


class LoopShallowX2(Scheme):
    """dlesm_shallow_step_x2_dm (section 8.1 row 7, event-ordered): TWO leapfrog steps and ONE depth-2 exchange per call on a
    halo_width-2 grid, twelve fields, rotation (cur, old, new1, new2) <- (new2, new1, old, cur).  Oracle: two steps, each
    followed by a depth-2 exchange; level n+2 is compared (level n+1 exists on the grown box only)"""
    names = LoopShallow.names + ["unew2", "vnew2", "pnew2"]
    depth = 2

    def __init__(self, g, t, oc, ncalls):
        self.g = g
        pts = {"u": D.GO_U_POINTS, "v": D.GO_V_POINTS, "p": D.GO_T_POINTS}
        self.F = {n: D.r2d_field(g, pts[n[0]]) for n in self.names}
        it = self.it = self.F["p"].internal
        self.box0 = (it.xstart - 1, it.xstop - 1, it.ystart - 1, it.ystop - 1)
        H = {}
        for k, n in enumerate(self.names):
            if k < 6:
                h = O.hash_field(SEED + 300 + k, g.ny, g.nx, 0, 0, 1, g.nx, 1, g.ny)
                h *= 0.01
                h += 1.0 if n[0] == "p" else -0.005
                assert O.exchange_all([h], [g.nx], [oc]) == 0
            else:
                h = np.full((g.ny, g.nx), 9.0)
            H[n] = h
        self.init = {n: torch.from_numpy(H[n]).cuda() for n in self.names}
        self.prm = D.psy.shallow_params(1.0e5, 1.0e5, 20.0)
        nm = self.names
        cur, old, new1, new2 = nm[0:3], nm[3:6], nm[6:9], nm[9:12]
        self.record(tuple(H[n] for n in cur))
        for _ in range(ncalls):
            for a, b, c in ((cur, old, new1), (new1, cur, new2)):
                O.sw_step(self.prm, g.nx, it.box(), *[H[n] for n in a + b], *[H[n] for n in c])
                for n in c:
                    assert O.exchange_all([H[n]], [g.nx], [oc]) == 0
            cur, old, new1, new2 = new2, new1, old, cur
            self.record(tuple(H[n] for n in cur))
        assert np.isfinite(H[cur[2]]).all()
        assert_every_handed_word_changes(self.frames, f"two-step shallow water on {it.nx}x{it.ny}")

    def reset(self, s):
        with torch.cuda.stream(s):
            for n in self.names:
                self.F[n].data.copy_(self.init[n])

    def step(self, k, form, s):
        nm = self.names
        cur, old, new1, new2 = (nm[0:3], nm[3:6], nm[6:9], nm[9:12]) if k % 2 == 0 else (nm[9:12], nm[6:9], nm[3:6], nm[0:3])
        D.psy.invoke_shallow_step_x2_dm(self.prm, *[self.F[n] for n in cur + old + new1 + new2], stream=s)
        return tuple(self.F[n].data for n in new2)

    def join(self, s):
        D.psy.halo_join(self.g, stream=s)

    def final_region(self):
        it = self.it
        m = np.zeros((self.g.ny, self.g.nx), dtype=bool)          # the box and its depth-2 halos
        m[it.ystart - 3:it.ystop + 2, it.xstart - 3:it.xstop + 2] = True
        return m


class LoopNemolite(Scheme):
    """dlesm_nemolite_step_dm (section 8.1 row 8, stream-ordered): the one-call NEMOLite2D-class step and the exchange of its
    five outputs over the mailboxes (three fields a turn), raw (ny, ld) arrays on a box with a one-cell ring, all cells wet,
    every input and grid array with the periodic halos of the loop-back plan.  Rotation after every step:
    (un, vn, sshn_t, sshn_u, sshn_v) <-> (ua, va, ssha, ssha_u, ssha_v).  Oracle: the CPU restatements in the order of
    tests/nemolite_step_dm_worker.py -- continuity, the exchange of ssha, next_sshu / next_sshv, momentum, the exchange of the
    five outputs.  A level = the five outputs."""
    PRM = (20.0, 0.00015, 50.0, 9.80665)          # rdt, cbfr, visc, g
    METRICS = ("dx_t", "dy_t", "dx_u", "dy_u", "dx_v", "dy_v", "area_t", "area_u", "area_v")
    INS = ("un", "vn", "ht", "hu", "hv", "sshn_t", "sshn_u", "sshn_v")
    OUTS = ("ssha", "ssha_u", "ssha_v", "ua", "va")
    MOM = ("un", "vn", "ht", "sshn_t", "hu", "sshn_u", "hv", "sshn_v", "ssha_u", "ssha_v")
    SWAP = {"un": "ua", "vn": "va", "sshn_t": "ssha", "sshn_u": "ssha_u", "sshn_v": "ssha_v"}

    def __init__(self, nx, ny, nsteps):
        import math
        import types

        import momentum_numpy as M
        from dl_esm_inf_amd import grid_mod
        from dm_overhead import loopback_tables
        ld, nyy = self.ld, self.ny = nx + 2, ny + 2
        box = self.box = (2, ld - 1, 2, nyy - 1)
        self.box0 = (1, nx, 1, ny)
        t = loopback_tables(D, D._cabi.Region(nx, ny, *box), 1)
        oc = O.Comms()
        C.memmove(C.byref(oc), C.byref(t), C.sizeof(oc))
        rng = np.random.default_rng(77 + ld)
        H = {k: 0.05 * rng.normal(size=(nyy, ld)) for k in ("un", "vn")}
        for k in ("ht", "hu", "hv"):
            H[k] = 10.0 + rng.random((nyy, ld))
        for k in ("sshn_t", "sshn_u", "sshn_v"):
            H[k] = 0.05 * rng.normal(size=(nyy, ld))
        G = {}
        for name in self.METRICS:
            a = 900.0 + 200.0 * rng.random((nyy, ld))
            G[name] = a * 1000.0 if name.startswith("area") else a
        G["fcor_u"] = M.coriolis(40.0 + 20.0 * rng.random((nyy, ld)), 7.292116e-5, math.pi / 180.0)
        G["fcor_v"] = M.coriolis(40.0 + 20.0 * rng.random((nyy, ld)), 7.292116e-5, math.pi / 180.0)
        for a in list(H.values()) + list(G.values()):
            assert O.exchange_all([a], [ld], [oc]) == 0
        for k in self.OUTS:
            H[k] = np.full((nyy, ld), -7.0)
        tm = np.ones((nyy, ld), dtype=np.int32)
        # ---- the device side: arrays, grid properties, a plan connected for three fields
        self.init = {k: torch.from_numpy(H[k]).cuda() for k in H}
        self.T = {k: torch.empty_like(v) for k, v in self.init.items()}
        self.gdev = {k: torch.from_numpy(v).cuda() for k, v in G.items()}
        self.gdev["tmask"] = torch.from_numpy(tm).cuda()
        self.mg = D._cabi.MomentumGrid(**{k: self.gdev[k].data_ptr() for k in M.GRID_ARRAYS})
        self.prm = D.psy.momentum_params(*self.PRM)
        self.plan = C.c_void_p()
        D._cabi.check(L.dlesm_halo_plan_create(C.byref(t), ld, nyy, C.byref(self.plan)))
        grid_mod.connect_peers(types.SimpleNamespace(_halo_plan=self.plan), 3)
        assert L.dlesm_halo_plan_peer_connected(self.plan) == 1
        # ---- the oracle's history
        Gn = M.SimpleNamespace(tmask=tm, **G)
        hp = M.params(*self.PRM)
        self.record(tuple(H[self.SWAP[k]] for k in ("sshn_t", "sshn_u", "sshn_v", "un", "vn")))     # (sentinels: level 0 is not compared)
        self.frames = []                                                                             # ... nor counted
        for _ in range(nsteps):
            O.continuity(self.PRM[0], ld, box, H["sshn_t"], H["sshn_u"], H["sshn_v"], H["hu"], H["hv"], H["un"], H["vn"],
                         G["area_t"], H["ssha"])
            assert O.exchange_all([H["ssha"]], [ld], [oc]) == 0
            M.next_sshu(box, tm, G["area_t"], G["area_u"], H["ssha"], H["ssha_u"])
            M.next_sshv(box, tm, G["area_t"], G["area_v"], H["ssha"], H["ssha_v"])
            M.momentum(hp, Gn, box, box, *[H[k] for k in self.MOM], H["ua"], H["va"])
            for k in self.OUTS:
                assert O.exchange_all([H[k]], [ld], [oc]) == 0
            self.record(tuple(H[k] for k in self.OUTS))
            for a, b in self.SWAP.items():
                H[a], H[b] = H[b], H[a]
        assert all(np.isfinite(H[k]).all() for k in H) and float(np.abs(H["un"]).max()) > 0.0
        assert len(self.frames) == nsteps
        assert_every_handed_word_changes(self.frames, f"NEMOLite2D step on {nx}x{ny}")
        self.frames.insert(0, None)            # (run() counts the levels: level 0 + one per step)

    def reset(self, s):
        with torch.cuda.stream(s):
            for k, v in self.init.items():
                self.T[k].copy_(v)

    def step(self, k, form, s):
        name = (lambda q: q) if k % 2 == 0 else (lambda q: {**self.SWAP, **{b: a for a, b in self.SWAP.items()}}.get(q, q))
        ins = [self.T[name(q)] for q in self.INS]
        outs = [self.T[name(q)] for q in self.OUTS]
        R = C.byref(D._cabi.Region(0, 0, *self.box))
        D._cabi.check(L.dlesm_nemolite_step_dm(self.plan, C.byref(self.prm), C.byref(self.mg), C.c_void_p(self.gdev["area_t"].data_ptr()),
                                               self.ld, self.ny, R, R, R, None, 0.0, *[C.c_void_p(t.data_ptr()) for t in ins + outs],
                                               C.c_void_p(s.cuda_stream)))
        return tuple(outs)

    def join(self, s):
        D._cabi.check(L.dlesm_halo_plan_join(self.plan, C.c_void_p(s.cuda_stream)))

    def final_region(self):
        return np.ones((self.ny, self.ld), dtype=bool)

    def close(self):
        D._cabi.check(L.dlesm_halo_plan_destroy(self.plan))


def loopback(tiles):
    from dm_overhead import loopback_tables
    D.parallel_init(0, 1, use_rccl=True)
    for name in tiles:
        nx, ny = (int(v) for v in name.split("x"))
        alignment, nsteps = TILES[name]
        g = make_grid(nx, ny, alignment)
        probe = D.r2d_field(g, D.GO_T_POINTS)
        t = loopback_tables(D, probe.internal)
        oc = O.Comms()
        C.memmove(C.byref(oc), C.byref(t), C.sizeof(oc))
        plans = {}
        for tr in ("rccl", "mailbox"):
            plans[tr] = C.c_void_p()
            D._cabi.check(L.dlesm_halo_plan_create(C.byref(t), g.nx, g.ny, C.byref(plans[tr])))
        D._cabi.check(L.dlesm_halo_plan_peer_connect_rccl(plans["mailbox"], 3))
        assert L.dlesm_halo_plan_peer_connected(plans["rccl"]) == 0 and L.dlesm_halo_plan_peer_connected(plans["mailbox"]) == 1
        small = nx * ny <= BIG
        J = LoopJacobi(g, t, oc, nsteps, "jacobi")
        X = LoopJacobi(g, t, oc, nsteps, "exchange")
        n9 = S9_STEPS.get(name, nsteps)
        S9 = LoopJacobi(g, t, oc, n9, "stencil9") if small else None
        SW = LoopShallow(g, t, oc, nsteps) if small else None
        for tr in ("rccl", "mailbox"):
            J.plan = X.plan = plans[tr]
            g._halo_plan = plans[tr]                       # (what the psy layer's shallow-water wrappers and halo_join use)
            tag = f"{name}/{tr}"
            if tr == "rccl":
                J.run(f"{tag}/jacobi-joined", "joined", nsteps)                                    # section 8.1 rows 1, 2
                J.run(f"{tag}/jacobi-time-loop-chain1", "pipelined", nsteps, (("j5_dm_chain", 1),))  # row 3
                J.run(f"{tag}/jacobi-time-loop-chain0", "pipelined", nsteps, (("j5_dm_chain", 0),))
            else:
                J.run(f"{tag}/jacobi-joined-fused1", "joined", nsteps, (("dm_peer_join_fused", 1),))  # row 4
                J.run(f"{tag}/jacobi-joined-fused0", "joined", nsteps, (("dm_peer_join_fused", 0),))
                J.run(f"{tag}/jacobi-time-loop", "pipelined", nsteps)
                X.run(f"{tag}/exchange-masks", "exchange", nsteps)
            if small:
                SW.run(f"{tag}/shallow-joined", "joined", nsteps)
                SW.run(f"{tag}/shallow-time-loop", "pipelined", nsteps)
                if tr == "rccl":
                    S9.plan = plans[tr]
                    S9.run(f"{tag}/stencil9", "stencil9", n9)
        g._halo_plan = None
        del J, X, S9, SW
        if small:                                          # row 7: the event-ordered two-step entry, over the mailboxes
            g2 = make_grid(nx, ny, alignment, hw=2)
            p2 = D.r2d_field(g2, D.GO_T_POINTS)
            t2 = loopback_tables(D, p2.internal, 2)
            oc2 = O.Comms()
            C.memmove(C.byref(oc2), C.byref(t2), C.sizeof(oc2))
            plan2 = C.c_void_p()
            D._cabi.check(L.dlesm_halo_plan_create(C.byref(t2), g2.nx, g2.ny, C.byref(plan2)))
            g2._halo_plan = plan2
            D.psy.halo_connect_peers(g2, 3)
            X2 = LoopShallowX2(g2, t2, oc2, nsteps // 2)
            # dm_skip_parts = 1: no RCCL group, only the mailboxes move halos; sw_x2_dm_overlap = 1: the frame-overlapped order,
            # which is the event-ordered hand-over of row 7 (frame launches, event, exchange on the side stream, interior, wait)
            X2.run(f"{name}/mailbox/shallow-x2", "x2", nsteps // 2, (("dm_skip_parts", 1),))
            if nx > 4 and ny > 4:      # (a tile without an interior behind its 2-deep frame takes the default order anyway)
                X2.run(f"{name}/mailbox/shallow-x2-overlapped", "x2", nsteps // 2, (("dm_skip_parts", 1), ("sw_x2_dm_overlap", 1)))
            g2._halo_plan = None
            del X2
            D._cabi.check(L.dlesm_halo_plan_destroy(plan2))
            # row 8: the stream-ordered NEMOLite2D-class step, over the mailboxes
            nn = min(nsteps, NEMO_STEPS)
            NM = LoopNemolite(nx, ny, nn)
            NM.run(f"{name}/mailbox/nemolite-step", "nemolite", nn, (("dm_skip_parts", 1),))
            NM.close()
            del NM
        for p in plans.values():
            D._cabi.check(L.dlesm_halo_plan_destroy(p))
        torch.cuda.empty_cache()


# =========================================================================================================== ranks mode
class RankScheme(Scheme):
    """this rank's tile of a scheme stepped on the UNDIVIDED domain by the oracle (fixed boundary ring)"""

    def window(self, a):
        it, gx0, gy0 = self.it, self.gx0, self.gy0
        return a[gy0 + it.ystart - 2:gy0 + it.ystop + 1, gx0 + it.xstart - 2:gx0 + it.xstop + 1]

    def setup_tile(self, g, fld):
        self.g = g
        it = self.it = fld.internal
        sub = g.subdomain
        self.gx0 = sub.glob.xstart - sub.internal.xstart + 1      # global index of local cell 1 (psy.hash_init)
        self.gy0 = sub.glob.ystart - sub.internal.ystart + 1
        self.box0 = (1, it.nx, 1, it.ny)                          # the internal region inside window()
        self.ring = D._cabi.Region(0, 0, it.xstart - 1, it.xstop + 1, it.ystart - 1, it.ystop + 1)

    def local(self, t):
        it = self.it
        return t[it.ystart - 2:it.ystop + 1, it.xstart - 2:it.xstop + 1]

    def join(self, s):
        D.psy.halo_join(self.g, stream=s)


class RankJacobi(RankScheme):
    def __init__(self, g, NX, NY, nsteps):
        self.x, self.y = D.r2d_field(g, D.GO_T_POINTS), D.r2d_field(g, D.GO_T_POINTS)
        self.setup_tile(g, self.x)
        gld = NX + 2
        G = O.hash_field(SEED, NY + 2, gld, 0, 0, 1, NX + 2, 1, NY + 2)
        Hh = G.copy()
        self.record((self.window(G),))
        for _ in range(nsteps):
            O.jacobi5(G, Hh, gld, 2, NX + 1, 2, NY + 1)
            G, Hh = Hh, G
            self.record((self.window(G),))
        assert_every_handed_word_changes(self.frames, f"jacobi, tile {self.it.nx}x{self.it.ny} of {NX}x{NY}")

    def reset(self, s):
        D.psy.hash_init(self.x, SEED, box=self.ring, stream=s)
        D.psy.hash_init(self.y, SEED, box=self.ring, stream=s)

    def step(self, k, form, s):
        a, b = (self.x, self.y) if k % 2 == 0 else (self.y, self.x)
        (D.psy.invoke_jacobi5_dm if form == "joined" else D.psy.invoke_jacobi5_dm_pipelined)(b, a, stream=s)
        return (self.local(b.data),)

    def final_region(self):
        m = np.ones((self.it.ny + 2, self.it.nx + 2), dtype=bool)     # internal region + the four edge halos (no corner travels)
        m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = False
        return m


class RankShallow(RankScheme):
    names = LoopShallow.names

    def __init__(self, g, NX, NY, nsteps):
        pts = {"u": D.GO_U_POINTS, "v": D.GO_V_POINTS, "p": D.GO_T_POINTS}
        self.F = {n: D.r2d_field(g, pts[n[0]]) for n in self.names}
        self.setup_tile(g, self.F["p"])
        gld = NX + 2
        HG = {}
        for k, nm in enumerate(self.names):
            hg = O.hash_field(SEED + 200 + k, NY + 2, gld, 0, 0, 1, NX + 2, 1, NY + 2)
            hg *= 0.01
            hg += 1.0 if nm[0] == "p" else -0.005
            HG[nm] = hg
        self.prm = D.psy.shallow_params(1.0e5, 1.0e5, 20.0)
        cur, old, new = self.names[:3], self.names[3:6], self.names[6:]
        self.record(tuple(self.window(HG[q]) for q in cur))
        for _ in range(nsteps):
            O.sw_step(self.prm, gld, (2, NX + 1, 2, NY + 1), *[HG[q] for q in cur + old], *[HG[q] for q in new])
            cur, old, new = new, cur, old
            self.record(tuple(self.window(HG[q]) for q in cur))
        assert np.isfinite(HG[cur[2]]).all()
        assert_every_handed_word_changes(self.frames, f"shallow water, tile {self.it.nx}x{self.it.ny} of {NX}x{NY}")

    def reset(self, s):
        with torch.cuda.stream(s):
            for k, nm in enumerate(self.names):
                D.psy.hash_init(self.F[nm], SEED + 200 + k, box=self.ring, stream=s)
                self.F[nm].data.mul_(0.01)
                self.F[nm].data.add_(1.0 if nm[0] == "p" else -0.005)

    def step(self, k, form, s):
        return tuple(self.local(t) for t in LoopShallow.step(self, k, form, s))

    def final_region(self):
        return np.ones((self.it.ny + 2, self.it.nx + 2), dtype=bool)   # internal region + the whole ring (nine-point footprint)


def ranks(domains, mode):
    if mode == "mailbox":
        D.parallel_init(rank, world, transport="mailbox")     # plans connect their own mailboxes (room for 3 fields)
    else:
        D.parallel_init(rank, world, use_rccl=False)            # the host program connects them (halo_connect_peers)
    for dom in domains.split(","):            # NXxNY:alignment
        size, align = dom.split(":")
        NX, NY = (int(v) for v in size.split("x"))
        if align == "none":
            os.environ.pop("DL_ESM_ALIGNMENT", None)
        else:
            os.environ["DL_ESM_ALIGNMENT"] = align
        g = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
        g.decompose(NX, NY)
        D.grid_init(g, 1.0, 1.0)
        D.psy.halo_connect_peers(g, 3)        # (mailbox mode: already connected when the plan was made -- a no-op)
        tag = f"{world}x{NX}x{NY}/{mode}"
        J = RankJacobi(g, NX, NY, RANK_STEPS["jacobi"])
        J.run(f"{tag}/jacobi-joined", "joined", RANK_STEPS["jacobi"])
        J.run(f"{tag}/jacobi-time-loop", "pipelined", RANK_STEPS["jacobi"])
        del J
        SW = RankShallow(g, NX, NY, RANK_STEPS["shallow"])
        SW.run(f"{tag}/shallow-alternating", "alternate", RANK_STEPS["shallow"])
        del SW


if MODE == "loopback":
    tiles = list(TILES)
    args = sys.argv[2:]
    while args:
        if args[0] == "--tiles":
            tiles = args[1].split(",")
        elif args[0] == "--tune":                # (scripts/handover_load_probe.py: the measurement-only reader forms)
            k, v = args[1].split("=")
            TUNING_DEFAULTS.setdefault(k, 1)
            tune(k, int(v))
        else:
            raise SystemExit(f"unknown argument {args[0]}")
        args = args[2:]
    loopback(tiles)
else:
    ranks(sys.argv[2], sys.argv[3])

if L.dlesm_ipc_open_retries():
    error(f"hipIpcOpenMemHandle had to be retried {L.dlesm_ipc_open_retries()} time(s)")
if L.dlesm_wait_timed_out(0):
    error("a device-side wait gave up")
for key in sorted(touched):
    L.dlesm_set_tuning(key.encode(), TUNING_DEFAULTS[key])
total = errors
if MODE == "ranks":
    tt = torch.tensor([errors])
    dist.all_reduce(tt)
    dist.barrier()
    total = int(tt.item())
print(f"rank {rank}: handover worker {MODE}: {nforms} forms, errors {errors} (all ranks {total})", flush=True)
if MODE == "ranks":
    D.parallel_finalise()
    dist.destroy_process_group()
sys.exit(1 if total else 0)
