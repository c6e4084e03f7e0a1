"""The flow step's own stability check (dlesm_flow_courant_async_f64) at 4096^2 and 8192^2, in one
process, by scripts/tracer_courant_probe.py's method: ms per call as medians of interleaved windows (device events around each
window, every variant warmed up first), closed basin, DL_ESM_ALIGNMENT=64.  Timed beside it in the same windows on the same
arrays: one dlesm_tracer_courant_async_f64 call.  That call is the yardstick: it reads 76 B/cell against 52 here, re-reads more
rows and divides more often, so the new check should not take longer; the allowance is the yardstick's own window-to-window
spread, max / median of its windows, which is recorded with the verdict.  The check's time is also given as GB/s under its
byte model, 52 B/cell read (mask 4 + six doubles) and nothing written -- a count of the bytes the algorithm needs, not of the
traffic the sweep causes (the mask's and vn's neighbouring rows are re-reads).  The record of the last call is printed with the
result.  Writes profiles/r19_flow_courant.json and prints the LAB_NOTES table.
    python scripts/flow_courant_probe.py [OUT.json] [WINDOWS] [N ...]"""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dl_esm_inf_amd as D  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r19_flow_courant.json"
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 7
sizes = [int(a) for a in sys.argv[3:]] or [4096, 8192]
FLOW_B, RDT, G, VISC = 52, 20.0, 9.80665, 100.0
torch.cuda.set_device(0)
os.environ["DL_ESM_ALIGNMENT"] = "64"
D.parallel_init(0, 1)
L = D._cabi.lib()
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
result = {"what": "ms per call, medians of interleaved windows (device events around each window): flow = one "
                  "dlesm_flow_courant_async_f64 call, tracer = one dlesm_tracer_courant_async_f64 call on the same arrays (the "
                  "yardstick); GB/s of the new check under its byte model (52 B/cell read, nothing written; the neighbouring "
                  "rows of the mask and of vn are re-reads); flow_over_tracer is judged against tracer_spread = max / median "
                  "of the yardstick's own windows",
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
    names = ("un", "vn", "ht", "hu", "hv", "sshn_t", "sshn_u", "sshn_v")
    F = {k: D.r2d_field(g, p) for k, p in zip(names, (U, V, T, U, V, T, U, V))}
    with torch.cuda.stream(s):                                         # (the scaling on the stream that fills the fields)
        for k, f in F.items():
            D.psy.hash_init(f, 90 + len(k), stream=s)
            f.data.mul_(0.01)
            if k in ("ht", "hu", "hv"):
                f.data.add_(10.0)
    it = F["sshn_t"].internal
    cells = (it.xstop - it.xstart + 1) * (it.ystop - it.ystart + 1)
    rec_f = torch.zeros(16, dtype=torch.float64, device="cuda")
    rec_t = torch.zeros(8, dtype=torch.float64, device="cuda")
    box = (g.nx, g.ny, it.xstart, it.xstop, it.ystart, it.ystop)
    args_f = (RDT, G, VISC, *box, g.tmask_device_ptr, C.c_void_p(g.dx_t_device.data_ptr()),
              C.c_void_p(g.dy_t_device.data_ptr()), *[F[k].device_ptr for k in ("un", "vn", "ht", "sshn_t")], 1.0, 1.0, 0.25, 0.0,
              C.c_void_p(rec_f.data_ptr()), sp)
    args_t = (RDT, *box, g.tmask_device_ptr, C.c_void_p(g.area_t_device.data_ptr()),
              *[F[k].device_ptr for k in ("un", "vn", "hu", "hv", "ht", "sshn_t", "sshn_u", "sshn_v")], 0.5, 1.0,
              C.c_void_p(rec_t.data_ptr()), sp)

    variants = {
        "flow": lambda: D._cabi.check(L.dlesm_flow_courant_async_f64(*args_f)),
        "tracer": lambda: D._cabi.check(L.dlesm_tracer_courant_async_f64(*args_t)),
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
    record = D._cabi.FlowCourant.from_buffer_copy(rec_f.cpu().numpy().tobytes())
    gbs = FLOW_B * cells / med["flow"] / 1e6
    spread = max(times["tracer"]) / med["tracer"]
    ratio = med["flow"] / med["tracer"]
    r = {"extents": [g.nx, g.ny], "cells": cells, "launches_per_window": launches, "ms": med, "ms_all_windows": times,
         "flow_model_bytes": FLOW_B, "flow_gbs": gbs, "flow_over_tracer": ratio, "tracer_spread": spread,
         "not_longer_than_the_tracer_check": bool(ratio <= spread), "record": list(record.as16())}
    result["sizes"][str(n)] = r
    print("%d^2: %r" % (n, record), flush=True)
    print("| N | flow check, ms | GB/s (52 B/cell) | tracer check, ms | flow / tracer | tracer check's max / median |")
    print("|---|---|---|---|---|---|")
    print("| %d | %.4f | %.0f | %.4f | %.3f | %.3f |" % (n, med["flow"], gbs, med["tracer"], ratio, spread), flush=True)
    del F, g, variants, rec_f, rec_t
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", out_path)
