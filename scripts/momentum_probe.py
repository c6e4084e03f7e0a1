"""Momentum kernels at 4096^2 and 8192^2: ms per launch of momentum_u, momentum_v, the fused entry
and next_sshu, and the 8-read + 1-write stream copy of libdlesm_lab.so in the same process, as medians of interleaved
windows; fractions of the 8 TB/s spec at 140 B/cell (each separate entry), 180 B/cell (fused) and 36 B/cell (next_ssh*).
    python scripts/momentum_probe.py [OUT.json] [WINDOWS]
--pmc: three launches of each entry at 8192^2 and nothing else, for a counter run of its own:
    rocprofv3 --pmc FETCH_SIZE WRITE_SIZE -d DIR -- python scripts/momentum_probe.py --pmc"""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

import dl_esm_inf_amd as D  # noqa: E402

PEAK = 8.0e12
PMC = sys.argv[1:2] == ["--pmc"]
out_path = sys.argv[1] if len(sys.argv) > 1 and not PMC else "profiles/r05_momentum.json"
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 7
torch.cuda.set_device(0)
os.environ["DL_ESM_ALIGNMENT"] = "64"
D.parallel_init(0, 1)
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
result = {"what": "ms per launch, medians of interleaved windows (device events around each window)", "windows": windows,
          "bytes_per_cell": {"momentum_u": 140, "momentum_v": 140, "momentum_fused": 180, "next_sshu": 36, "copy_8r1w": 72},
          "device": torch.cuda.get_device_name(0), "sizes": {}}

for n in ((8192,) if PMC else (4096, 8192)):
    g = D.grid_type(D.GO_ARAKAWA_C, (1, 1, 2), D.GO_OFFSET_NE)
    g.decompose(n, n)
    D.grid_init(g, 1000.0, 1000.0)
    D.psy.coriolis(g)
    T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
    F = [D.r2d_field(g, p) for p in (U, V, T, T, U, U, V, V, U, V)]   # un, vn, ht, sshn_t, hu, sshn_u, hv, sshn_v, ssha_u, ssha_v
    for k, f in enumerate(F):
        D.psy.hash_init(f, 70 + k, stream=s)
        if k in (2, 4, 6):
            f.data.add_(10.0)                                           # depths
    ua, va, su = D.r2d_field(g, U), D.r2d_field(g, V), D.r2d_field(g, U)
    for name in ("dx_t", "dy_t", "dx_u", "dy_u", "dx_v", "dy_v", "area_t", "area_u", "area_v"):
        getattr(g, name + "_device")
    prm = D.psy.momentum_params(20.0, 0.00015, 50.0, 9.80665)
    cells = ua.internal.xstop - ua.internal.xstart + 1
    cells *= ua.internal.ystop - ua.internal.ystart + 1
    nc = (g.nx * g.ny) & ~1
    srcs = (C.c_void_p * 8)(*[F[k].device_ptr for k in range(8)])
    dsts = (C.c_void_p * 1)(ua.device_ptr)
    variants = {
        "momentum_u": lambda: D.psy.invoke_momentum_u(prm, ua, *F[:9], stream=s),
        "momentum_v": lambda: D.psy.invoke_momentum_v(prm, va, *F[:8], F[9], stream=s),
        "momentum_fused": lambda: D.psy.invoke_momentum(prm, ua, va, *F, stream=s),
        "next_sshu": lambda: D.psy.invoke_next_sshu(su, F[3], stream=s),
        "copy_8r1w": lambda: D._cabi.check_lab(D._cabi.lab().dlesm_lab_stream_copy_f64(8, 1, srcs, dsts, nc, 0, sp)),
    }
    if PMC:
        with torch.cuda.stream(s):
            for fn in variants.values():
                for _ in range(3):
                    fn()
        s.synchronize()
        print("pmc launches done", flush=True)
        sys.exit(0)
    launches = 20 if n == 4096 else 10
    times = {k: [] for k in variants}
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
    byts = result["bytes_per_cell"]
    frac = {k: byts[k] * (nc if k == "copy_8r1w" else cells) / (med[k] * 1e-3) / PEAK for k in med}
    r = {"cells": cells, "launches_per_window": launches, "ms": med, "ms_all_windows": times, "frac_of_8TBps": frac,
         "fused_over_separate": med["momentum_fused"] / (med["momentum_u"] + med["momentum_v"]),
         "fused_frac_of_copy_8r1w": frac["momentum_fused"] / frac["copy_8r1w"]}
    result["sizes"][str(n)] = r
    print(n, json.dumps({k: round(v, 4) for k, v in med.items()}), "frac", json.dumps({k: round(v, 3) for k, v in frac.items()}),
          "fused/separate %.3f" % r["fused_over_separate"], flush=True)
    del F, ua, va, su, g
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", out_path)
