#!/usr/bin/env python3
"""Price the coupled step on a decomposed grid (dlesm_nemolite_coupled_step_dm) on ONE GPU, in
loop-back (rank 0 is its own eight neighbours), closed basin with an island, on a grid decomposed with halo_width = 2.
ms per time step of:

    coupled    dlesm_nemolite_coupled_step_dm with the Hancock scheme and K tracers on a depth-2 loop-back plan: the ssha
               ring kernel, the single-domain step, the tracer sweep, ONE exchange of the 5 + K outputs
    separate   what the library offered before, on the same arrays: dlesm_nemolite_step_dm on a depth-1 loop-back plan over
               the same box, then dlesm_tracer_step_hancock_dm on the depth-2 plan (two exchanges)

each over the RCCL group and over the mailboxes (the plans connected for three fields).  Every row is a time loop with the
step's rotation (the tracers' buffers swap too): a warm-up, then a fixed number of calls between two events on the caller's
stream; rows are measured --reps times, interleaved (row by row, round after round), every window is recorded, the median and
the fastest window are reported with the spread (max - min) / min of each row.  No target: the entry saves one exchange, and
an exchange is about 2 % of a step.

    python scripts/coupled_dm_probe.py [--tiles 8192] [--tracers 2] [--calls 30] [--warmup 5] [--reps 7] [--out OUT.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

PRM = (20.0, 0.00015, 50.0, 9.80665)
INS = ("un", "vn", "ht", "hu", "hv", "sshn_t", "sshn_u", "sshn_v")
OUTS = ("ssha", "ssha_u", "ssha_v", "ua", "va")
FLOW = ("un", "vn", "hu", "hv", "ht", "sshn_t", "sshn_u", "sshn_v", "ssha")
HANCOCK = 2


def make(D, L, tile, ntracers, peer):
    import torch
    from dm_overhead import loopback_tables
    g = D.grid_type(D.GO_ARAKAWA_C, (1, 1, 2), D.GO_OFFSET_NE)
    g.decompose(tile, tile, halo_width=2)
    D.grid_init(g, 1000.0, 1000.0)
    it = g.subdomain.internal
    g.tmask[it.ystart - 1 + tile // 3:it.ystart - 1 + tile // 3 + 64, it.xstart - 1 + tile // 2:it.xstart - 1 + tile // 2 + 96] = 0
    g._tmask_device = None                                                      # an island; the mirror is made from it
    D.psy.coriolis(g)
    T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
    pts = {"ssha": T, "sshn_t": T, "ht": T, "sshn_u": U, "ssha_u": U, "un": U, "ua": U, "hu": U,
           "sshn_v": V, "ssha_v": V, "vn": V, "va": V, "hv": V}
    F = {k: D.r2d_field(g, p) for k, p in pts.items()}
    for k in ("ht", "hu", "hv"):
        D.set_field(F[k], 10.0)
    jj, ii = torch.meshgrid(torch.arange(g.ny, device="cuda", dtype=torch.float64),
                            torch.arange(g.nx, device="cuda", dtype=torch.float64), indexing="ij")
    F["sshn_t"].data.copy_(0.01 * torch.exp(-((ii - 0.6 * tile) ** 2 + (jj - 0.5 * tile) ** 2) / (2 * 60.0 ** 2)))
    Cin, Cout = [], []
    for n in range(ntracers):
        a, b = D.r2d_field(g, T), D.r2d_field(g, T)
        a.data.copy_(1.0 + n + 0.5 * torch.sin(ii / 37.0) * torch.cos(jj / 53.0))
        b.data.copy_(a.data)
        Cin.append(a)
        Cout.append(b)
    del ii, jj
    plans = []
    for depth in (1, 2):
        t = loopback_tables(D, F["ssha"].internal, depth)
        plan = C.c_void_p()
        D._cabi.check(L.dlesm_halo_plan_create(C.byref(t), g.nx, g.ny, C.byref(plan)))
        if peer:
            D._cabi.check(L.dlesm_halo_plan_peer_connect_rccl(plan, 3))
        plans.append(plan)
    return g, F, Cin, Cout, plans


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, nargs="+", default=[8192])
    ap.add_argument("--tracers", type=int, default=2)
    ap.add_argument("--calls", type=int, default=30, help="timed calls per window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7, help="interleaved rounds over all rows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_coupled_dm.json"))
    args = ap.parse_args()
    import torch
    import dl_esm_inf_amd as D
    L = D._cabi.lib()
    ck = D._cabi.check
    torch.cuda.set_device(0)
    os.environ["DL_ESM_ALIGNMENT"] = "64"
    D.parallel_init(0, 1, use_rccl=True)
    prm = D.psy.momentum_params(*PRM)
    K = args.tracers
    out = {"unit": "ms per time step", "calls": args.calls, "warmup": args.warmup, "reps": args.reps, "alignment": 64,
           "tracers": K, "scheme": "hancock",
           "model": "closed basin with an island, halo_width = 2, loop-back depth-2 plan (separate: the flow step on a "
                    "depth-1 loop-back plan over the same box)", "rows": {}}

    def window(fn):
        for _ in range(args.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.calls

    rows = {}
    for tile in args.tiles:
        for peer in (0, 1):
            g, F, Cin, Cout, (plan1, plan2) = make(D, L, tile, K, peer)
            mg = D.psy._momentum_grid(g, "probe")
            area_t = C.c_void_p(g.area_t_device.data_ptr())
            R = [C.byref(F[k].internal) for k in ("ssha", "ua", "va")]
            it = F["ssha"].internal
            state = {"A": {k: F[k].device_ptr for k in F}, "ci": [f.device_ptr for f in Cin], "co": [f.device_ptr for f in Cout]}

            def ptrs(v):
                return (C.c_void_p * max(len(v), 1))(*[p.value for p in v])

            def rot():
                A = state["A"]
                for a, b in (("un", "ua"), ("vn", "va"), ("sshn_t", "ssha"), ("sshn_u", "ssha_u"), ("sshn_v", "ssha_v")):
                    A[a], A[b] = A[b], A[a]
                state["ci"], state["co"] = state["co"], state["ci"]

            def coupled():
                A = state["A"]
                ck(L.dlesm_nemolite_coupled_step_dm(plan2, None, HANCOCK, C.byref(prm), C.byref(mg), area_t, g.nx, g.ny, *R,
                                                    None, 0.0, *[A[k] for k in INS], *[A[k] for k in OUTS], ptrs(state["ci"]),
                                                    ptrs(state["co"]), K, None))
                rot()

            def separate():
                A = state["A"]
                ck(L.dlesm_nemolite_step_dm(plan1, C.byref(prm), C.byref(mg), area_t, g.nx, g.ny, *R, None, 0.0,
                                            *[A[k] for k in INS], *[A[k] for k in OUTS], None))
                ck(L.dlesm_tracer_step_hancock_dm(plan2, prm.rdt, g.nx, g.ny, it.xstart, it.xstop, it.ystart, it.ystop,
                                                  C.c_void_p(mg.tmask), area_t, *[A[k] for k in FLOW], ptrs(state["ci"]),
                                                  ptrs(state["co"]), K, None))
                rot()

            fns = {"coupled": coupled, "separate": separate}
            key = f"{tile}_{'mailbox' if peer else 'rccl'}"
            rows[key] = {n: [] for n in fns}
            for _ in range(args.reps):
                for n, fn in fns.items():
                    rows[key][n].append(window(fn))
            torch.cuda.synchronize()
            assert L.dlesm_wait_timed_out(0) == 0
            for plan in (plan1, plan2):
                ck(L.dlesm_halo_plan_destroy(plan))
            del F, Cin, Cout
            torch.cuda.empty_cache()

    for key, r in rows.items():
        med = {n: sorted(v)[len(v) // 2] for n, v in r.items()}
        out["rows"][key] = {
            "windows": r,
            "median": med,
            "min": {n: min(v) for n, v in r.items()},
            "spread": {n: (max(v) - min(v)) / min(v) for n, v in r.items()},
            "coupled_over_separate": med["coupled"] / med["separate"],
        }
        o = out["rows"][key]
        print(f"{key}: coupled {med['coupled']:.4f}  separate {med['separate']:.4f}  "
              f"coupled/separate {o['coupled_over_separate']:.3f}  spread(coupled) {o['spread']['coupled']:.3f}  "
              f"spread(separate) {o['spread']['separate']:.3f}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    assert all(math.isfinite(v) for r in out["rows"].values() for v in r["median"].values())


if __name__ == "__main__":
    main()
