"""GPU test (-m gpu) that pins what the distributed stencil and shallow-water steps refuse, and in which order:
dlesm_jacobi5_step_dm, dlesm_jacobi5_step_dm_pipelined, dlesm_stencil9_step_dm, dlesm_jacobi5_multi_step_dm, the four
dlesm_shallow_step*_dm* and the two *_x2_dm.  Every refusal keeps its return code and its WHOLE text; where two can be
triggered at once the one that is reported is pinned.  What tests/test_gpu_shallow_refusals.py pins for the shallow-water
entries (null plan, null q, a plan of other extents, the box, the overlaps) is not repeated: here they get the one refusal
that file does not reach -- a send strip off the one-cell ring on a plan connected to its mailboxes -- and the two-step
entries their own wrong-depth text.

One process, loop-back on one GPU: 16 x 14 arrays with the 12 x 10 box (3:14, 3:12), a depth-1 plan, a depth-2 plan, a
depth-1 plan made for 18 x 14 arrays, and two depth-1 plans connected to their mailboxes (for one field and for three).
Nothing is launched by a refusal: after all of them every array holds what it held.  Then ONE successful call per entry
on the plans that have just refused, against the same entry's single-domain twin followed by dlesm_halo_exchange_multi_f64
on the same plan, bit for bit in all twelve arrays: a refusal leaves the plan usable.  (The twin of a two-step entry is its
definition -- the single-domain step over the box grown by one cell, then over the box -- because the single-domain two-step
entries have no neighbour's cells to compute.)  The texts are literals written from the format strings.

Not exercised: the timed-out refusal (reaching it means making a wait give up) and the stream-capture refusal (it depends
on the installed RCCL)."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

LD, NY = 16, 14
BOX, INNER = (3, 14, 3, 12), (4, 13, 4, 11)
EBOX = (2, 15, 2, 13)               # the last stage box of the fused Jacobi step on a tile with eight neighbours
SENTINEL = 9.0
ALPHA = 0.001

J5, J5P, S9, MULTI = "dlesm_jacobi5_step_dm", "dlesm_jacobi5_step_dm_pipelined", "dlesm_stencil9_step_dm", "dlesm_jacobi5_multi_step_dm"
SW, SWP, SWS, SWSP = ("dlesm_shallow_step_dm", "dlesm_shallow_step_dm_pipelined", "dlesm_shallow_step_smooth_dm",
                      "dlesm_shallow_step_smooth_dm_pipelined")
X2, X2S = "dlesm_shallow_step_x2_dm", "dlesm_shallow_step_smooth_x2_dm"

NULLP = "null pointer"
EXTENTS = "plan is for 18x14 fields, got 16x14"
NSTEPS = "fused distributed step: nsteps = %d (2..8 supported)"
MULTI_DEPTH = "the plan exchanges depth-%d halos, the fused step needs depth %d"
X2_DEPTH = "%s: the plan exchanges depth-1 halos, two steps per launch need depth 2 (dlesm_map_comms_depth, depth = 2)"
# the first send of the sorted lists: direction 1, the west column of the internal region
FRAME = ("peer transport: send strip (3:3,3:12) is not part of the one-cell frame of the box (plans of halo depth 1 stepped "
         "over their internal region only)")
RING = ("peer transport: send strip (3:3,3:12) is not part of the one-cell ring of the box (plans of halo depth 1 stepped "
        "over their internal region only)")


@pytest.fixture(scope="module")
def D():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    import dl_esm_inf_amd as d
    torch.cuda.set_device(0)
    d.parallel_init(0, 1, use_rccl=True)
    return d


def test_every_refusal_keeps_its_code_and_its_text_and_leaves_the_plan_usable(D):
    import torch
    from dm_overhead import loopback_tables
    L = D._cabi.lib()
    check, Region = D._cabi.check, D._cabi.Region
    prm = D.psy.shallow_params(1.0e5, 1.0e5, 90.0)
    coef = (C.c_double * 9)(0.0625, 0.125, 0.0625, 0.125, 0.25, 0.125, 0.0625, 0.125, 0.03125)
    rng = np.random.default_rng(LD * NY)
    host = [rng.random((NY, LD)) * 0.01 + (1.0 if k % 3 == 2 else -0.005) for k in range(6)]
    host += [np.full((NY, LD), SENTINEL) for _ in range(6)]
    dev = [torch.from_numpy(h).cuda() for h in host]
    ptr = [t.data_ptr() for t in dev]

    it = Region(12, 10, *BOX)
    t1, t2 = loopback_tables(D, it, 1), loopback_tables(D, it, 2)
    plan1, plan2, other, peer1, peer3 = (C.c_void_p() for _ in range(5))
    for p, t, ld in ((plan1, t1, LD), (plan2, t2, LD), (other, t1, 18), (peer1, t1, LD), (peer3, t1, LD)):
        check(L.dlesm_halo_plan_create(C.byref(t), ld, NY, C.byref(p)))
    D.psy.halo_connect_peers(types.SimpleNamespace(_halo_plan=peer1), 1)
    D.psy.halo_connect_peers(types.SimpleNamespace(_halo_plan=peer3), 3)
    assert L.dlesm_halo_plan_peer_connected(peer1) == 1 and L.dlesm_halo_plan_peer_connected(peer3) == 1
    null = C.c_void_p(0)

    def vp(k):
        return C.c_void_p(k) if k else None

    def exchange(plan, ks, mask=D._cabi.DIRS_ALL):
        return L.dlesm_halo_exchange_multi_f64(plan, (C.c_void_p * len(ks))(*[ptr[k] for k in ks]), len(ks), mask, None)

    # the six inputs with valid depth-2 halos (which holds the depth-1 ring of the same wrap); what every run starts from
    check(exchange(plan2, [0, 1, 2, 3, 4, 5]))
    torch.cuda.synchronize()
    base = [t.cpu().clone() for t in dev]

    def jacobi(e, plan, box=BOX, a=ptr[2], b=ptr[6]):
        return getattr(L, e)(plan, vp(a), vp(b), LD, NY, *box, None)

    def stencil9(plan, box=BOX, a=ptr[2], b=ptr[6], c=coef):
        return L.dlesm_stencil9_step_dm(plan, vp(a), vp(b), c, LD, NY, *box, None)

    def multi(plan, nsteps=2, a=ptr[2], b=ptr[6]):
        return L.dlesm_jacobi5_multi_step_dm(plan, vp(a), vp(b), LD, NY, nsteps, *BOX, None)

    def shallow(e, plan, box=BOX, q=True):
        a = [plan, C.byref(prm) if q else None] + ([ALPHA] if "smooth" in e else [])
        return getattr(L, e)(*a, LD, NY, *box, *[vp(k) for k in ptr[:12 if "x2" in e else 9]], None)

    cases = []          # (what, call, the whole text)

    def case(what, fn, text):
        cases.append((what, fn, text))

    for e in (J5, J5P):
        case(e + ": a null plan", lambda e=e: jacobi(e, null), NULLP)
        case(e + ": a null in", lambda e=e: jacobi(e, plan1, a=0), NULLP)
        case(e + ": a null out", lambda e=e: jacobi(e, plan1, b=0), NULLP)
        case(e + ": a plan of other extents", lambda e=e: jacobi(e, other), EXTENTS)
        case(e + ": a strip off the frame", lambda e=e: jacobi(e, peer1, box=INNER), FRAME)
        # order
        case(e + ": a null in and a plan of other extents", lambda e=e: jacobi(e, other, a=0), NULLP)
        case(e + ": a null out and a strip off the frame", lambda e=e: jacobi(e, peer1, box=INNER, b=0), NULLP)
    case(S9 + ": a null plan", lambda: stencil9(null), NULLP)
    case(S9 + ": a null in", lambda: stencil9(plan1, a=0), NULLP)
    case(S9 + ": a null out", lambda: stencil9(plan1, b=0), NULLP)
    case(S9 + ": null coefficients", lambda: stencil9(plan1, c=None), NULLP)
    case(S9 + ": a plan of other extents", lambda: stencil9(other), EXTENTS)
    case(S9 + ": null coefficients and a plan of other extents", lambda: stencil9(other, c=None), NULLP)
    case(MULTI + ": a null plan", lambda: multi(null), NULLP)
    case(MULTI + ": a null in", lambda: multi(plan2, a=0), NULLP)
    case(MULTI + ": a null out", lambda: multi(plan2, b=0), NULLP)
    case(MULTI + ": a plan of other extents", lambda: multi(other), EXTENTS)
    for n in (1, 9, 0, -1):
        case(MULTI + ": nsteps = %d" % n, lambda n=n: multi(plan2, nsteps=n), NSTEPS % n)
    case(MULTI + ": a depth-1 plan", lambda: multi(plan1), MULTI_DEPTH % (1, 2))
    case(MULTI + ": a depth-2 plan and three steps", lambda: multi(plan2, nsteps=3), MULTI_DEPTH % (2, 3))
    # order
    case(MULTI + ": a null in and a plan of other extents", lambda: multi(other, a=0), NULLP)
    case(MULTI + ": a plan of other extents and nsteps = 1", lambda: multi(other, nsteps=1), EXTENTS)
    case(MULTI + ": nsteps = 9 and a depth-1 plan", lambda: multi(plan1, nsteps=9), NSTEPS % 9)
    for e in (SW, SWP, SWS, SWSP):
        case(e + ": a strip off the ring", lambda e=e: shallow(e, peer3, box=INNER), RING)
        case(e + ": a null q and a strip off the ring", lambda e=e: shallow(e, peer3, box=INNER, q=False), NULLP)
    for e in (X2, X2S):
        case(e + ": a depth-1 plan", lambda e=e: shallow(e, plan1), X2_DEPTH % e)
    assert len(cases) == 2 * 7 + 6 + (4 + 4 + 2 + 3) + 4 * 2 + 2

    def snapshot():
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in dev]

    def compare(what, run, twin, plan, ks, mask=D._cabi.DIRS_ALL, join=False):
        """the entry against its twin + exchange of arrays `ks`, every array whole"""
        for t, b in zip(dev, base):
            t.copy_(b)
        check(run())
        if join:
            check(L.dlesm_halo_plan_join(plan, None))
        got = snapshot()
        for t, b in zip(dev, base):
            t.copy_(b)
        check(twin())
        check(exchange(plan, ks, mask))
        want = snapshot()
        for k, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), (what, k, np.argwhere(g != w)[:5])
        assert not np.array_equal(got[ks[0]], base[ks[0]].numpy()), what       # (something was computed)

    def stencil5():
        return L.dlesm_stencil5_f64(vp(ptr[2]), vp(ptr[6]), LD, NY, *BOX, None)

    def step(e, box, ks, tmp=()):
        """a single-domain one-step entry on arrays ks; 'T' stands for the three scratch arrays tmp"""
        a = [C.byref(prm)] + ([ALPHA] if "smooth" in e else [])
        p9 = [t.data_ptr() for t in tmp] if "T" in ks else []
        return getattr(L, e)(*a, LD, NY, *box, *[vp(p9.pop(0) if k == "T" else ptr[k]) for k in ks], None)

    def twin_x2():      # level n+1 on the grown box, level n+2 on the box
        return (step("dlesm_shallow_step_f64", EBOX, range(9)) or
                step("dlesm_shallow_step_f64", BOX, (6, 7, 8, 0, 1, 2, 9, 10, 11)))

    def twin_x2s():     # T <- u, old2 <- old; T = level n+1 and old2 = filtered n on the grown box; new2 and filtered n+1 on the box
        tmp = [dev[k].clone() for k in range(3)]
        for k in range(3):
            dev[9 + k].copy_(dev[3 + k])
        rc = (step("dlesm_shallow_step_smooth_f64", EBOX, (0, 1, 2, 9, 10, 11, "T", "T", "T"), tmp) or
              step("dlesm_shallow_step_smooth_f64", BOX, ("T", "T", "T", 9, 10, 11, 6, 7, 8), tmp))
        torch.cuda.synchronize()
        return rc

    plans = (plan1, plan2, other, peer1, peer3)
    try:
        bad = []
        for what, fn, text in cases:
            rc = fn()
            err = L.dlesm_last_error()
            if rc != D._cabi.EINVAL or err != text.encode():
                bad.append((what, rc, err, text))
        assert not bad, bad
        for k, (g, b) in enumerate(zip(snapshot(), base)):
            assert np.array_equal(g, b.numpy()), ("a refusal wrote array", k)

        edges = D._cabi.DIRS_EDGES_ONLY         # a 5-point stencil reads no corner: the Jacobi steps exchange the four edges
        for plan, name in ((plan1, "rccl"), (peer1, "mailboxes")):
            for e in (J5, J5P):
                compare(e + " " + name, lambda: jacobi(e, plan), stencil5, plan, [6], edges, join=e == J5P)
        compare(S9, lambda: stencil9(plan1), lambda: L.dlesm_stencil9_f64(vp(ptr[2]), vp(ptr[6]), coef, LD, NY, *BOX, None),
                plan1, [6])
        compare(MULTI, lambda: multi(plan2),
                lambda: L.dlesm_stencil5_multi_f64(vp(ptr[2]), vp(ptr[6]), LD, NY, 2, *BOX, *EBOX, 1, 1, 1, 1, None), plan2, [6])
        for plan, name in ((plan1, "rccl"), (peer3, "mailboxes")):
            for e in (SW, SWP, SWS, SWSP):
                single = "dlesm_shallow_step_smooth_f64" if "smooth" in e else "dlesm_shallow_step_f64"
                compare(e + " " + name, lambda: shallow(e, plan), lambda: step(single, BOX, range(9)), plan, [6, 7, 8],
                        join=e.endswith("pipelined"))
        compare(X2, lambda: shallow(X2, plan2), twin_x2, plan2, [9, 10, 11])
        compare(X2S, lambda: shallow(X2S, plan2), twin_x2s, plan2, [6, 7, 8, 9, 10, 11])
        assert L.dlesm_wait_timed_out(0) == 0
    finally:
        for p in plans:
            L.dlesm_halo_plan_destroy(p)
