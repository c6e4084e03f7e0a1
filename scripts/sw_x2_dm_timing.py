#!/usr/bin/env python3
"""Price two shallow-water steps per call on a decomposed grid (dlesm_shallow_step_x2_dm / _smooth_x2_dm) on ONE GPU, in
loop-back (rank 0 is its own eight neighbours), against the forms a decomposed model has without them.  ms per TIME STEP of:

    x2_dm_overlap / x2_dm_serial      the new entry: 2-deep frame strips + exchange behind the interior / whole box, then exchange
    dm_pipelined                      dlesm_shallow_step_dm_pipelined, one step per call (a halo_width-1 grid, its own plan)
    x2_single                         dlesm_shallow_step_x2_f64 on the same tile, no exchange at all (the ceiling)

and the same three for the filtered forms (smooth_x2_dm_*, smooth_dm_pipelined, smooth_x2_single), each over the RCCL group
and over the mailboxes (the plan connected for three fields).  Every row is a time loop with the entry's own rotation: a
warm-up, then a fixed number of calls between two events on the caller's stream; the rows are measured --reps times,
interleaved (row by row, round after round), every window is recorded, and the fastest and the median window are reported
with the spread (max - min) / min of each row.

    python scripts/sw_x2_dm_timing.py [--tiles 4096 8192] [--calls 50] [--warmup 10] [--reps 7] [--out profiles/r05_sw_x2_dm_loopback.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

NAMES = ["u", "v", "p", "uold", "vold", "pold", "unew", "vnew", "pnew", "unew2", "vnew2", "pnew2"]
ALPHA = 0.1


def make_grid(D, L, tile, hw, peer):
    """a tile of a decomposed grid (halo_width hw), its twelve fields and a loop-back plan of depth hw"""
    from dm_overhead import loopback_tables
    g = D.grid_type(D.GO_ARAKAWA_C, (1, 1, 2), D.GO_OFFSET_NE)
    g.decompose(tile, tile, halo_width=hw)
    D.grid_init(g, 1.0, 1.0)
    pts = {"u": D.GO_U_POINTS, "v": D.GO_V_POINTS, "p": D.GO_T_POINTS}
    F = {n: D.r2d_field(g, pts[n[0]]) for n in NAMES}
    t = loopback_tables(D, F["p"].internal, hw)
    plan = C.c_void_p()
    D._cabi.check(L.dlesm_halo_plan_create(C.byref(t), g.nx, g.ny, C.byref(plan)))
    g._halo_plan = plan
    if peer:
        D._cabi.check(L.dlesm_halo_plan_peer_connect_rccl(plan, 3))
    return g, F, plan


def fill(D, F):
    for k, n in enumerate(NAMES):
        D.psy.hash_init(F[n], 900 + k)
        F[n].data.mul_(0.01)
        F[n].data.add_(1.0 if n[0] == "p" else -0.005)
    D.psy.halo_exchange_multi([F["u"], F["v"], F["p"]])
    D.psy.halo_exchange_multi([F["uold"], F["vold"], F["pold"]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, nargs="+", default=[4096, 8192])
    ap.add_argument("--calls", type=int, default=50, help="timed calls per window")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7, help="interleaved rounds over all rows")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05_sw_x2_dm_loopback.json"))
    args = ap.parse_args()
    import torch
    import dl_esm_inf_amd as D
    L = D._cabi.lib()
    torch.cuda.set_device(0)
    os.environ["DL_ESM_ALIGNMENT"] = "64"
    D.parallel_init(0, 1, use_rccl=True)
    prm = D.psy.shallow_params(1.0e5, 1.0e5, 90.0)
    out = {"unit": "ms per time step", "calls": args.calls, "warmup": args.warmup, "reps": args.reps, "alpha": ALPHA, "alignment": 64,
           "rows": {}}

    def window(fn, steps_per_call, join=None):
        for _ in range(args.warmup):
            fn()
        if join:
            join()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            fn()
        if join:
            join()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (args.calls * steps_per_call)

    for tile in args.tiles:
        for transport in ("rccl", "mailbox"):
            peer = transport == "mailbox"
            g2, F2, plan2 = make_grid(D, L, tile, 2, peer)
            g1, F1, plan1 = make_grid(D, L, tile, 1, peer)
            fill(D, F2)
            fill(D, F1)
            rows = {}

            def rot4(F):
                s = {"cur": [F[n] for n in ("u", "v", "p")], "old": [F[n] for n in ("uold", "vold", "pold")],
                     "n1": [F[n] for n in ("unew", "vnew", "pnew")], "n2": [F[n] for n in ("unew2", "vnew2", "pnew2")]}

                def advance():
                    s["cur"], s["old"], s["n1"], s["n2"] = s["n2"], s["n1"], s["old"], s["cur"]
                return s, advance

            def ping(F):
                s = {"a": [F[n] for n in ("u", "v", "p", "uold", "vold", "pold")],
                     "b": [F[n] for n in ("unew2", "vnew2", "pnew2", "unew", "vnew", "pnew")]}

                def advance():
                    s["a"], s["b"] = s["b"], s["a"]
                return s, advance

            def x2_dm(overlap):
                s, adv = rot4(F2)

                def fn():
                    L.dlesm_set_tuning(b"sw_x2_dm_overlap", overlap)
                    D.psy.invoke_shallow_step_x2_dm(prm, *s["cur"], *s["old"], *s["n1"], *s["n2"])
                    adv()
                return fn

            def smooth_x2_dm(overlap):
                s, adv = ping(F2)

                def fn():
                    L.dlesm_set_tuning(b"sw_x2_dm_overlap", overlap)
                    D.psy.invoke_shallow_step_smooth_x2_dm(prm, ALPHA, *s["a"], *s["b"])
                    adv()
                return fn

            def x2_single():
                s, adv = rot4(F2)

                def fn():
                    D.psy.invoke_shallow_step_x2(prm, *s["cur"], *s["old"], *s["n1"], *s["n2"])
                    adv()
                return fn

            def smooth_x2_single():
                s, adv = ping(F2)

                def fn():
                    D.psy.invoke_shallow_step_smooth_x2(prm, ALPHA, *s["a"], *s["b"])
                    adv()
                return fn

            def dm_pipelined():
                s = {"c": [F1[n] for n in ("u", "v", "p")], "o": [F1[n] for n in ("uold", "vold", "pold")],
                     "n": [F1[n] for n in ("unew", "vnew", "pnew")]}

                def fn():
                    D.psy.invoke_shallow_step_dm_pipelined(prm, *s["c"], *s["o"], *s["n"])
                    s["c"], s["o"], s["n"] = s["n"], s["c"], s["o"]
                return fn

            def smooth_dm_pipelined():
                s = {"c": [F1[n] for n in ("u", "v", "p")], "o": [F1[n] for n in ("uold", "vold", "pold")],
                     "n": [F1[n] for n in ("unew", "vnew", "pnew")]}

                def fn():   # the filtered old level is updated in place: (cur, old, new) <- (new, old, cur)
                    D.psy.invoke_shallow_step_smooth_dm(prm, ALPHA, *s["c"], *s["o"], *s["n"], pipelined=True)
                    s["c"], s["n"] = s["n"], s["c"]
                return fn

            join1 = lambda: D.psy.halo_join(g1)      # noqa: E731
            cases = [("x2_single", x2_single(), 2, None), ("x2_dm_overlap", x2_dm(1), 2, None),
                     ("x2_dm_serial", x2_dm(0), 2, None), ("dm_pipelined", dm_pipelined(), 1, join1),
                     ("smooth_x2_single", smooth_x2_single(), 2, None), ("smooth_x2_dm_overlap", smooth_x2_dm(1), 2, None),
                     ("smooth_x2_dm_serial", smooth_x2_dm(0), 2, None), ("smooth_dm_pipelined", smooth_dm_pipelined(), 1, join1)]
            for rep in range(args.reps):
                for name, fn, spc, join in cases:
                    rows.setdefault(name, []).append(window(fn, spc, join))
            L.dlesm_set_tuning(b"sw_x2_dm_overlap", 0)
            best = {k: min(v) for k, v in rows.items()}
            median = {k: sorted(v)[len(v) // 2] for k, v in rows.items()}
            spread = {k: (max(v) - min(v)) / min(v) for k, v in rows.items()}
            res = {"ms_per_step": best, "ms_per_step_median": median, "spread": spread, "windows": rows}
            res["x2_dm_best_vs_single"] = best["x2_single"] / min(best["x2_dm_overlap"], best["x2_dm_serial"])
            res["x2_dm_best_vs_dm_pipelined"] = best["dm_pipelined"] / min(best["x2_dm_overlap"], best["x2_dm_serial"])
            res["smooth_x2_dm_best_vs_single"] = best["smooth_x2_single"] / min(best["smooth_x2_dm_overlap"],
                                                                                best["smooth_x2_dm_serial"])
            res["smooth_x2_dm_best_vs_dm_pipelined"] = best["smooth_dm_pipelined"] / min(best["smooth_x2_dm_overlap"],
                                                                                          best["smooth_x2_dm_serial"])
            out["rows"][f"{tile}_{transport}"] = res
            print(json.dumps({f"{tile}_{transport}": res}), flush=True)
            for g, plan in ((g2, plan2), (g1, plan1)):
                D.psy.halo_join(g)
                torch.cuda.synchronize()
                D._cabi.check(L.dlesm_halo_plan_destroy(plan))
                g._halo_plan = None
            del F1, F2
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
