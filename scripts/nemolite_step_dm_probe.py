#!/usr/bin/env python3
"""Price the one-call NEMOLite2D-class step on a decomposed grid (dlesm_nemolite_step_dm) on ONE GPU, in
loop-back (rank 0 is its own eight neighbours through depth-1 tables), closed basin with an island.  ms per time step of:

    dm            dlesm_nemolite_step_dm: the ssha ring kernel, the single-domain step, one exchange of the five outputs
    single        dlesm_nemolite_step_f64 on the same tile, no exchange (the ceiling)
    single_xchg   dlesm_nemolite_step_f64 + the five-field exchange as the dm call issues it (dm less its ring kernel)
    definition    continuity, the ssha exchange, next_sshu, next_sshv, momentum, the five-field exchange

each over the RCCL group and over the mailboxes (the plan connected for three fields: the five outputs in two turns).  Every
row is a time loop with the step's rotation: a warm-up, then a fixed number of calls between two events on the caller's
stream; rows are measured --reps times, interleaved (row by row, round after round), every window is recorded, the median
and the fastest window are reported with the spread (max - min) / min of each row.  The ring kernel's own time comes from a
kernel trace of this script (rocprofv3 --kernel-trace --stats), not from these windows.

    python scripts/nemolite_step_dm_probe.py [--tiles 4096 8192] [--calls 30] [--warmup 5] [--reps 7] [--out OUT.json]
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
MOM = ("un", "vn", "ht", "sshn_t", "hu", "sshn_u", "hv", "sshn_v", "ssha_u", "ssha_v")


def make(D, L, tile, peer):
    import numpy as np
    import torch
    from dm_overhead import loopback_tables
    g = D.grid_type(D.GO_ARAKAWA_C, (1, 1, 2), D.GO_OFFSET_NE)
    g.decompose(tile, tile)
    user = np.ones((tile + 2, tile + 2), dtype=np.int32)
    user[tile // 3:tile // 3 + 64, tile // 2:tile // 2 + 96] = 0               # an island
    D.grid_init(g, 1000.0, 1000.0, tmask=user)
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
    t = loopback_tables(D, F["ssha"].internal, 1)
    plan = C.c_void_p()
    D._cabi.check(L.dlesm_halo_plan_create(C.byref(t), g.nx, g.ny, C.byref(plan)))
    g._halo_plan = plan
    if peer:
        D._cabi.check(L.dlesm_halo_plan_peer_connect_rccl(plan, 3))
    return g, F, plan


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--calls", type=int, default=30, help="timed calls per window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7, help="interleaved rounds over all rows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_nemolite_step_dm.json"))
    args = ap.parse_args()
    import torch
    import dl_esm_inf_amd as D
    L = D._cabi.lib()
    ck = D._cabi.check
    torch.cuda.set_device(0)
    os.environ["DL_ESM_ALIGNMENT"] = "64"
    D.parallel_init(0, 1, use_rccl=True)
    prm = D.psy.momentum_params(*PRM)
    out = {"unit": "ms per time step", "calls": args.calls, "warmup": args.warmup, "reps": args.reps, "alignment": 64,
           "model": "closed basin with an island, loop-back depth-1 plan", "rows": {}}

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
            g, F, plan = make(D, L, tile, peer)
            mg = D.psy._momentum_grid(g, "probe")
            area_t = C.c_void_p(g.area_t_device.data_ptr())
            R = [C.byref(F[k].internal) for k in ("ssha", "ua", "va")]
            P = {k: F[k].device_ptr for k in F}
            turn = 3 if peer else 5
            state = {"A": dict(P)}

            def rot():
                A = state["A"]
                for a, b in (("un", "ua"), ("vn", "va"), ("sshn_t", "ssha"), ("sshn_u", "ssha_u"), ("sshn_v", "ssha_v")):
                    A[a], A[b] = A[b], A[a]

            def xchg5():
                A = state["A"]
                for k in range(0, 5, turn):
                    names = OUTS[k:k + turn]
                    arr = (C.c_void_p * len(names))(*[A[n] for n in names])
                    ck(L.dlesm_halo_exchange_multi_f64(plan, arr, len(names), D._cabi.DIRS_ALL, None))

            def dm():
                A = state["A"]
                ck(L.dlesm_nemolite_step_dm(plan, C.byref(prm), C.byref(mg), area_t, g.nx, g.ny, *R, None, 0.0,
                                            *[A[k] for k in INS], *[A[k] for k in OUTS], None))
                rot()

            def single():
                A = state["A"]
                ck(L.dlesm_nemolite_step_f64(C.byref(prm), C.byref(mg), area_t, g.nx, g.ny, *R, None, 0.0,
                                             *[A[k] for k in INS], *[A[k] for k in OUTS], None))
                rot()

            def single_xchg():
                A = state["A"]
                ck(L.dlesm_nemolite_step_f64(C.byref(prm), C.byref(mg), area_t, g.nx, g.ny, *R, None, 0.0,
                                             *[A[k] for k in INS], *[A[k] for k in OUTS], None))
                xchg5()
                rot()

            it = F["ssha"].internal

            def definition():
                A = state["A"]
                ck(L.dlesm_continuity_f64(prm.rdt, g.nx, g.ny, it.xstart, it.xstop, it.ystart, it.ystop,
                                          *[A[k] for k in ("sshn_t", "sshn_u", "sshn_v", "hu", "hv", "un", "vn")], area_t,
                                          A["ssha"], None))
                ck(L.dlesm_halo_exchange_f64(plan, A["ssha"], D._cabi.DIRS_ALL, None))
                ck(L.dlesm_next_sshu_f64(g.nx, g.ny, it.xstart, it.xstop, it.ystart, it.ystop, C.c_void_p(mg.tmask), area_t,
                                         C.c_void_p(mg.area_u), A["ssha"], A["ssha_u"], None))
                ck(L.dlesm_next_sshv_f64(g.nx, g.ny, it.xstart, it.xstop, it.ystart, it.ystop, C.c_void_p(mg.tmask), area_t,
                                         C.c_void_p(mg.area_v), A["ssha"], A["ssha_v"], None))
                ck(L.dlesm_momentum_f64(C.byref(prm), C.byref(mg), g.nx, g.ny, R[1], R[2], *[A[k] for k in MOM], A["ua"],
                                        A["va"], None))
                xchg5()
                rot()

            fns = {"dm": dm, "single": single, "single_xchg": single_xchg, "definition": definition}
            key = f"{tile}_{'mailbox' if peer else 'rccl'}"
            rows[key] = {n: [] for n in fns}
            for _ in range(args.reps):
                for n, fn in fns.items():
                    rows[key][n].append(window(fn))
            torch.cuda.synchronize()
            ck(L.dlesm_halo_plan_destroy(plan))
            g._halo_plan = None
            del F
            torch.cuda.empty_cache()

    for key, r in rows.items():
        med = {n: sorted(v)[len(v) // 2] for n, v in r.items()}
        out["rows"][key] = {
            "windows": r,
            "median": med,
            "min": {n: min(v) for n, v in r.items()},
            "spread": {n: (max(v) - min(v)) / min(v) for n, v in r.items()},
            "dm_over_single": med["dm"] / med["single"],
            "dm_over_definition": med["dm"] / med["definition"],
            "dm_less_single_xchg_ms": med["dm"] - med["single_xchg"],
            "exchange_ms": med["single_xchg"] - med["single"],
        }
        o = out["rows"][key]
        print(f"{key}: dm {med['dm']:.4f}  single {med['single']:.4f}  single+xchg {med['single_xchg']:.4f}  "
              f"definition {med['definition']:.4f}  dm/single {o['dm_over_single']:.3f}  "
              f"dm/definition {o['dm_over_definition']:.3f}  spread(dm) {o['spread']['dm']:.3f}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    assert all(math.isfinite(v) for r in out["rows"].values() for v in r["median"].values())


if __name__ == "__main__":
    main()
