"""Tracer transport in one sweep (dlesm_tracer_step_f64) at 4096^2 and 8192^2, in one process: ms per
call of ONE call carrying K = 1, 2, 4, 8 tracers against K calls carrying one tracer each, as medians of interleaved windows
(device events around each window), closed basin, DL_ESM_ALIGNMENT=64.  Each time is also given as GB/s under the byte model
of section 6.10 -- 84 B/cell of flow per launch (two launches beyond four tracers) + 16 B/cell per tracer -- beside the lab
library's copy ceiling measured in the same run on the same arrays (dlesm_lab_stream_copy_f64, 8 arrays read + 1 written).
The byte model counts the bytes the algorithm needs, not the traffic the sweep causes (it re-reads the rows above and below,
mostly from cache).  Writes profiles/r10_tracer.json and prints the LAB_NOTES table.
The second-order limited entry (dlesm_tracer_step_muscl_f64) is timed beside it in the same windows,
one call with K tracers: its compulsory bytes are the same 84 + 16 K B/cell (rows j-2 and j+2 are re-reads), so it is given
under the same byte model and as a ratio to the same-run upwind call.  Those rows go to profiles/r13_tracer_muscl.json
(TRACER_PROBE_MUSCL_OUT names another file).
The time-centred limited entry (dlesm_tracer_step_hancock_f64) is timed in the same windows too, under
the same byte model (its six extra rows of area_t, ht, sshn_t are re-reads) and as a ratio to the same-run limited call, whose
code it shares but for the face factors.  Those rows, with the same run's upwind and limited times beside them, go to
profiles/r14_tracer_hancock.json (TRACER_PROBE_HANCOCK_OUT names another file).
    python scripts/tracer_probe.py [OUT.json] [WINDOWS] [N ...]"""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dl_esm_inf_amd as D  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r10_tracer.json"
muscl_path = os.environ.get("TRACER_PROBE_MUSCL_OUT", "profiles/r13_tracer_muscl.json")
hancock_path = os.environ.get("TRACER_PROBE_HANCOCK_OUT", "profiles/r14_tracer_hancock.json")
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 7
sizes = [int(a) for a in sys.argv[3:]] or [4096, 8192]
KS = (1, 2, 4, 8)
FLOW_B, TRACER_B, COPY_B = 84, 16, 72
torch.cuda.set_device(0)
os.environ["DL_ESM_ALIGNMENT"] = "64"
D.parallel_init(0, 1)
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
result = {"what": "ms per K tracers, medians of interleaved windows (device events around each window): one = one "
                  "dlesm_tracer_step_f64 call with K tracers, split = K calls with one tracer each; GB/s under the byte model "
                  "(84 B/cell of flow per launch + 16 B/cell per tracer); copy = dlesm_lab_stream_copy_f64, 8 read + 1 written",
          "windows": windows, "device": torch.cuda.get_device_name(0), "sizes": {}}
muscl_result = {"what": "ms per K tracers, medians of the same interleaved windows: muscl = one dlesm_tracer_step_muscl_f64 "
                        "call with K tracers, upwind = one dlesm_tracer_step_f64 call with K tracers; GB/s under the same "
                        "byte model (rows j-2 and j+2 are re-reads); muscl_over_upwind = the ratio of the two times",
                "windows": windows, "device": result["device"], "sizes": {}}
hancock_result = {"what": "ms per K tracers, medians of the same interleaved windows: hancock = one "
                          "dlesm_tracer_step_hancock_f64 call with K tracers, muscl = one dlesm_tracer_step_muscl_f64 call, "
                          "upwind = one dlesm_tracer_step_f64 call; GB/s under the same byte model (the rows j-1 and j+1 of "
                          "area_t, ht, sshn_t are re-reads); hancock_over_muscl, muscl_over_upwind = ratios of the times",
                  "windows": windows, "device": result["device"], "sizes": {}}


def model_bytes(k, launches):
    return FLOW_B * launches + TRACER_B * k


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
    Ci, Co = [D.r2d_field(g, T) for _ in range(8)], [D.r2d_field(g, T) for _ in range(8)]
    for k, f in enumerate(Ci):
        D.psy.hash_init(f, 200 + k, stream=s)
    flow = [F[k] for k in names]
    it = F["ssha"].internal
    cells = (it.xstop - it.xstart + 1) * (it.ystop - it.ystart + 1)
    src = (C.c_void_p * 8)(*[F[k].device_ptr for k in names[:8]])
    dst = (C.c_void_p * 1)(Co[0].device_ptr)
    nc = (g.nx * g.ny) & ~1

    def one(k):
        return lambda: D.psy.invoke_tracer_step(20.0, Co[:k], Ci[:k], *flow, stream=s)

    def muscl(k):
        return lambda: D.psy.invoke_tracer_step_muscl(20.0, Co[:k], Ci[:k], *flow, stream=s)

    def hancock(k):
        return lambda: D.psy.invoke_tracer_step_hancock(20.0, Co[:k], Ci[:k], *flow, stream=s)

    def split(k):
        def fn():
            for m in range(k):
                D.psy.invoke_tracer_step(20.0, Co[m:m + 1], Ci[m:m + 1], *flow, stream=s)
        return fn

    variants = {"copy": lambda: D._cabi.check_lab(D._cabi.lab().dlesm_lab_stream_copy_f64(8, 1, src, dst, nc, 0, sp))}
    for k in KS:
        variants["one_%d" % k] = one(k)
        variants["split_%d" % k] = split(k)
        variants["muscl_%d" % k] = muscl(k)
        variants["hancock_%d" % k] = hancock(k)
    launches = 10
    times = {k: [] for k in variants}
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for fn in variants.values():                                   # warm-up: code objects, first touches
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
    copy_gbs = COPY_B * nc / med["copy"] / 1e6
    r = {"extents": [g.nx, g.ny], "cells": cells, "ms": med, "ms_all_windows": times, "copy_gbs": copy_gbs, "rows": []}
    print("%d^2: copy 8r+1w %.4f ms = %.0f GB/s" % (n, med["copy"], copy_gbs), flush=True)
    print("| K | one call, ms | GB/s (model B/cell) | K calls, ms | GB/s (model B/cell) | one / split | copy GB/s |")
    print("|---|---|---|---|---|---|---|")
    for k in KS:
        b1, bk = model_bytes(k, 1 if k <= 4 else 2), model_bytes(k, k)
        g1, gk = b1 * cells / med["one_%d" % k] / 1e6, bk * cells / med["split_%d" % k] / 1e6
        ratio = med["one_%d" % k] / med["split_%d" % k]
        r["rows"].append({"k": k, "one_ms": med["one_%d" % k], "one_model_bytes": b1, "one_gbs": g1,
                          "split_ms": med["split_%d" % k], "split_model_bytes": bk, "split_gbs": gk, "one_over_split": ratio})
        print("| %d | %.4f | %.0f (%d) | %.4f | %.0f (%d) | %.3f | %.0f |" % (k, med["one_%d" % k], g1, b1, med["split_%d" % k],
                                                                              gk, bk, ratio, copy_gbs), flush=True)
    result["sizes"][str(n)] = r
    rm = {"extents": [g.nx, g.ny], "cells": cells, "copy_gbs": copy_gbs, "rows": []}
    print("| K | limited, ms | GB/s (model B/cell) | upwind, ms | limited / upwind |")
    print("|---|---|---|---|---|")
    for k in KS:
        b1 = model_bytes(k, 1 if k <= 4 else 2)
        tm_, tu = med["muscl_%d" % k], med["one_%d" % k]
        rm["rows"].append({"k": k, "muscl_ms": tm_, "model_bytes": b1, "muscl_gbs": b1 * cells / tm_ / 1e6, "upwind_ms": tu,
                           "muscl_over_upwind": tm_ / tu})
        print("| %d | %.4f | %.0f (%d) | %.4f | %.3f |" % (k, tm_, b1 * cells / tm_ / 1e6, b1, tu, tm_ / tu), flush=True)
    muscl_result["sizes"][str(n)] = rm
    rh = {"extents": [g.nx, g.ny], "cells": cells, "copy_gbs": copy_gbs, "rows": [],
          "ms_all_windows": {k: v for k, v in times.items() if k.split("_")[0] in ("hancock", "muscl", "one")}}
    print("| K | time-centred, ms | GB/s (model B/cell) | limited, ms | upwind, ms | time-centred / limited | limited / upwind |")
    print("|---|---|---|---|---|---|---|")
    for k in KS:
        b1 = model_bytes(k, 1 if k <= 4 else 2)
        th, tm_, tu = med["hancock_%d" % k], med["muscl_%d" % k], med["one_%d" % k]
        rh["rows"].append({"k": k, "hancock_ms": th, "model_bytes": b1, "hancock_gbs": b1 * cells / th / 1e6, "muscl_ms": tm_,
                           "upwind_ms": tu, "hancock_over_muscl": th / tm_, "muscl_over_upwind": tm_ / tu})
        print("| %d | %.4f | %.0f (%d) | %.4f | %.4f | %.3f | %.3f |" % (k, th, b1 * cells / th / 1e6, b1, tm_, tu, th / tm_,
                                                                        tm_ / tu), flush=True)
    hancock_result["sizes"][str(n)] = rh
    del F, Ci, Co, flow, g, variants
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", out_path)
os.makedirs(os.path.dirname(muscl_path) or ".", exist_ok=True)
with open(muscl_path, "w") as f:
    json.dump(muscl_result, f, indent=1)
print("wrote", muscl_path)
os.makedirs(os.path.dirname(hancock_path) or ".", exist_ok=True)
with open(hancock_path, "w") as f:
    json.dump(hancock_result, f, indent=1)
print("wrote", hancock_path)
