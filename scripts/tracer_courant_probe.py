"""The tracer schemes' Courant check (dlesm_tracer_courant_async_f64) at 4096^2 and 8192^2, in one
process, by scripts/tracer_probe.py's method: ms per call as medians of interleaved windows (device events around each window,
every variant warmed up first), closed basin, DL_ESM_ALIGNMENT=64.  Timed beside it in the same windows on the same arrays: one
dlesm_tracer_step_f64 call and one dlesm_tracer_step_hancock_f64 call, each carrying one tracer.  The Hancock call is the
yardstick: it reads a superset of the check's arrays, does the same divisions and also writes, so the check should not take
longer.  The ratio to the upwind call is recorded, not judged.  The check's time is also given as GB/s under its byte model, 76
B/cell read (mask 4 + nine doubles) and nothing written -- a count of the bytes the algorithm needs, not of the traffic the
sweep causes (rows j-1 and j+1 are re-reads).  The record of the last call is printed with the result.
Writes profiles/r18_tracer_courant.json and prints the LAB_NOTES table.
    python scripts/tracer_courant_probe.py [OUT.json] [WINDOWS] [N ...]"""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dl_esm_inf_amd as D  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r18_tracer_courant.json"
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 7
sizes = [int(a) for a in sys.argv[3:]] or [4096, 8192]
COURANT_B, RDT = 76, 20.0
torch.cuda.set_device(0)
os.environ["DL_ESM_ALIGNMENT"] = "64"
D.parallel_init(0, 1)
L = D._cabi.lib()
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
result = {"what": "ms per call, medians of interleaved windows (device events around each window): courant = one "
                  "dlesm_tracer_courant_async_f64 call, upwind = one dlesm_tracer_step_f64 call with one tracer, hancock = one "
                  "dlesm_tracer_step_hancock_f64 call with one tracer; GB/s of the check under its byte model (76 B/cell "
                  "read, nothing written; rows j-1 and j+1 are re-reads); courant_over_hancock is the yardstick, "
                  "courant_over_upwind is recorded only",
          "windows": windows, "device": torch.cuda.get_device_name(0), "sizes": {}}

for n in sizes:
    user = np.ones((n + 2, n + 2), dtype=np.int32)
    user[0, :] = user[-1, :] = 0
    user[:, 0] = user[:, -1] = 0
    g = D.grid_type(D.GO_ARAKAWA_C, (1, 1, 2), D.GO_OFFSET_NE)
    g.decompose(n, n)
    D.grid_init(g, 1000.0, 1000.0, tmask=user)
    del user
    T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
    names = ("ssha", "un", "vn", "ht", "hu", "hv", "sshn_t", "sshn_u", "sshn_v")
    F = {k: D.r2d_field(g, p) for k, p in zip(names, (T, U, V, T, U, V, T, U, V))}
    for k, f in F.items():
        D.psy.hash_init(f, 90 + len(k), stream=s)
        f.data.mul_(0.01)
        if k in ("ht", "hu", "hv"):
            f.data.add_(10.0)
    Ci, Co = [D.r2d_field(g, T)], [D.r2d_field(g, T)]
    D.psy.hash_init(Ci[0], 200, stream=s)
    flow = [F[k] for k in names]
    it = F["sshn_t"].internal
    cells = (it.xstop - it.xstart + 1) * (it.ystop - it.ystart + 1)
    rec = torch.zeros(8, dtype=torch.float64, device="cuda")
    args = (RDT, g.nx, g.ny, it.xstart, it.xstop, it.ystart, it.ystop, g.tmask_device_ptr,
            C.c_void_p(g.area_t_device.data_ptr()),
            *[F[k].device_ptr for k in ("un", "vn", "hu", "hv", "ht", "sshn_t", "sshn_u", "sshn_v")], 0.5, 1.0,
            C.c_void_p(rec.data_ptr()), sp)

    variants = {
        "courant": lambda: D._cabi.check(L.dlesm_tracer_courant_async_f64(*args)),
        "upwind": lambda: D.psy.invoke_tracer_step(RDT, Co, Ci, *flow, stream=s),
        "hancock": lambda: D.psy.invoke_tracer_step_hancock(RDT, Co, Ci, *flow, stream=s),
    }
    launches = 60 if n <= 4096 else 20                                 # windows of tens of milliseconds
    times = {k: [] for k in variants}
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for fn in variants.values():                                   # warm-up: code objects, first touches, the scratch pool
            for _ in range(3):
                fn()
        for _ in range(windows):
            for k, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(launches):
                    fn()
                e1.record(s)
                s.synchronize()
                times[k].append(e0.elapsed_time(e1) / launches)
    med = {k: statistics.median(v) for k, v in times.items()}
    record = D._cabi.TracerCourant.from_buffer_copy(rec.cpu().numpy().tobytes())
    gbs = COURANT_B * cells / med["courant"] / 1e6
    r = {"extents": [g.nx, g.ny], "cells": cells, "launches_per_window": launches, "ms": med, "ms_all_windows": times,
         "courant_model_bytes": COURANT_B, "courant_gbs": gbs, "courant_over_hancock": med["courant"] / med["hancock"],
         "courant_over_upwind": med["courant"] / med["upwind"], "record": list(record.as8())}
    result["sizes"][str(n)] = r
    print("%d^2: %r" % (n, record), flush=True)
    print("| N | check, ms | GB/s (76 B/cell) | upwind K = 1, ms | Hancock K = 1, ms | check / Hancock | check / upwind |")
    print("|---|---|---|---|---|---|---|")
    print("| %d | %.4f | %.0f | %.4f | %.4f | %.3f | %.3f |" % (n, med["courant"], gbs, med["upwind"], med["hancock"],
                                                              r["courant_over_hancock"], r["courant_over_upwind"]), flush=True)
    del F, Ci, Co, flow, g, variants, rec
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", out_path)
