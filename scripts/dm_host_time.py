#!/usr/bin/env python3
"""Host time of one call of dlesm_jacobi5_step_dm_pipelined on ONE GPU in loop-back (rank 0 is its own neighbours): wall
time over `--calls` calls with nothing between them and no synchronisation, one join and one synchronise behind the window,
`--windows` windows, their median.  The tile is small (1024^2 by default), so the calls are launch-bound and the figure is
what the host spends issuing a step: the frame/interior launch, the side stream's wait + exchange + flag, the bookkeeping.
For A/B runs of two builds set DLESM_HIP_LIB (one process per build, interleaved).

    python scripts/dm_host_time.py [--tile 1024] [--calls 4000] [--windows 7] [--peer]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tile", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=4000)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--peer", action="store_true", help="connect the plan's mailboxes: the step takes the peer transport")
    args = ap.parse_args()
    import torch
    import dl_esm_inf_amd as D
    from dm_overhead import loopback_tables
    L = D._cabi.lib()
    torch.cuda.set_device(0)
    os.environ["DL_ESM_ALIGNMENT"] = "64"
    D.parallel_init(0, 1, use_rccl=True)
    g = D.grid_type(D.GO_ARAKAWA_C, (1, 1, 2), D.GO_OFFSET_NE)
    g.decompose(args.tile, args.tile)
    D.grid_init(g, 1.0, 1.0)
    a, b = D.r2d_field(g, D.GO_T_POINTS), D.r2d_field(g, D.GO_T_POINTS)
    tables = loopback_tables(D, a.internal)
    plan = C.c_void_p()
    D._cabi.check(L.dlesm_halo_plan_create(C.byref(tables), g.nx, g.ny, C.byref(plan)))
    if args.peer:
        D._cabi.check(L.dlesm_halo_plan_peer_connect_rccl(plan, 1))
    s = torch.cuda.Stream()
    sp = C.c_void_p(s.cuda_stream)
    box = a.internal.box()
    step = L.dlesm_jacobi5_step_dm_pipelined
    pa, pb, nx, ny = a.device_ptr, b.device_ptr, g.nx, g.ny
    D.psy.hash_init(a, 20261004, stream=s)
    D._cabi.check(L.dlesm_halo_exchange_f64(plan, a.device_ptr, D._cabi.DIRS_ALL, sp))
    D.copy_field(a, b, stream=s)
    us = []
    for w in range(args.windows + 1):                    # (the first window warms up and is dropped)
        s.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls // 2):
            rc = step(plan, pa, pb, nx, ny, *box, sp) or step(plan, pb, pa, nx, ny, *box, sp)
            if rc:
                D._cabi.check(rc)
        t1 = time.perf_counter()
        D._cabi.check(L.dlesm_halo_plan_join(plan, sp))
        s.synchronize()
        if w:
            us.append((t1 - t0) / (args.calls // 2 * 2) * 1e6)
    assert L.dlesm_wait_timed_out(0) == 0
    print(json.dumps({"tile": args.tile, "transport": "mailboxes" if args.peer else "rccl", "calls": args.calls // 2 * 2,
                      "host_us_per_call": {"median": statistics.median(us), "min": min(us), "max": max(us)},
                      "windows": [round(x, 3) for x in us]}))
    D._cabi.check(L.dlesm_halo_plan_destroy(plan))


if __name__ == "__main__":
    main()
