"""The model's output fields (dlesm_flow_output_f64) at 4096^2 and 8192^2, in one process, by
scripts/flow_courant_probe.py's method: ms per call as medians of interleaved windows (device events around each window,
every variant warmed up first), closed basin, DL_ESM_ALIGNMENT=64.  Timed in the same windows on the same arrays:
  set6    all six outputs, DLESM_OUT_SET            add6   all six outputs, DLESM_OUT_ADD
  set3    {UT, VT, SPEED}, DLESM_OUT_SET
  tracer  one dlesm_tracer_step_f64 call with one tracer -- the yardstick
  torch3  {UT, VT, SPEED} as the torch expressions a Python user writes today (no land selects)
Byte models, counts of the bytes the algorithms need and not of the traffic the sweeps cause (neighbouring rows and columns
are re-reads): set6 100 B/cell (mask 4, six doubles read, six written), add6 148 (the six outputs read as well), set3 44
(mask, un, vn; three written), the one-tracer upwind sweep 100 (84 + 16).  set6 should not take longer than the tracer sweep
by more than that sweep's own window-to-window spread, max / median of its windows, which is recorded with the verdict.  The
ratio to the torch form is recorded and nothing is promised for it.  Writes profiles/r20_flow_output.json and prints the
LAB_NOTES table.
    python scripts/flow_output_probe.py [OUT.json] [WINDOWS] [N ...]"""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dl_esm_inf_amd as D  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r20_flow_output.json"
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 7
sizes = [int(a) for a in sys.argv[3:]] or [4096, 8192]
BYTES = {"set6": 100, "add6": 148, "set3": 44, "tracer": 100}
RDT = 20.0
torch.cuda.set_device(0)
os.environ["DL_ESM_ALIGNMENT"] = "64"
D.parallel_init(0, 1)
L = D._cabi.lib()
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
result = {"what": "ms per call, medians of interleaved windows (device events around each window): set6 / add6 = one "
                  "dlesm_flow_output_f64 call with all six outputs in SET / ADD mode, set3 = {UT, VT, SPEED} in SET mode, "
                  "tracer = one dlesm_tracer_step_f64 call with one tracer on the same flow arrays (the yardstick), torch3 = "
                  "{UT, VT, SPEED} as torch expressions; GB/s under each byte model (model_bytes, B/cell; neighbouring rows "
                  "and columns are re-reads); set6_over_tracer is judged against tracer_spread = max / median of the "
                  "yardstick's own windows",
          "windows": windows, "device": torch.cuda.get_device_name(0), "model_bytes": BYTES, "sizes": {}}

for n in sizes:
    user = np.ones((n + 2, n + 2), dtype=np.int32)
    user[0, :] = user[-1, :] = 0
    user[:, 0] = user[:, -1] = 0
    g = D.grid_type(D.GO_ARAKAWA_C, (1, 1, 2), D.GO_OFFSET_NE)
    g.decompose(n, n)
    D.grid_init(g, 1000.0, 1000.0, tmask=user)
    del user
    T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
    names = ("un", "vn", "ht", "hu", "hv", "sshn_t", "sshn_u", "sshn_v", "ssha", "c_in", "c_out")
    F = {k: D.r2d_field(g, p) for k, p in zip(names, (U, V, T, U, V, T, U, V, T, T, T))}
    out = [D.r2d_field(g, T) for _ in range(D._cabi.OUT_COUNT)]
    with torch.cuda.stream(s):                                         # (the scaling on the stream that fills the fields)
        for k, f in F.items():
            D.psy.hash_init(f, 90 + len(k), stream=s)
            f.data.mul_(0.01)
            if k in ("ht", "hu", "hv"):
                f.data.add_(10.0)
    it = F["sshn_t"].internal
    cells = (it.xstop - it.xstart + 1) * (it.ystop - it.ystart + 1)
    box = (g.nx, g.ny, it.xstart, it.xstop, it.ystart, it.ystop)
    ins = (g.tmask_device_ptr, C.c_void_p(g.dx_v_device.data_ptr()), C.c_void_p(g.dy_u_device.data_ptr()),
           *[F[k].device_ptr for k in ("un", "vn", "ht", "sshn_t")])
    p6 = (C.c_void_p * 6)(*[f.device_ptr for f in out])
    p3 = (C.c_void_p * 6)(None, out[1].device_ptr, out[2].device_ptr, out[3].device_ptr, None, None)
    cin, cout = (C.c_void_p * 1)(F["c_in"].device_ptr), (C.c_void_p * 1)(F["c_out"].device_ptr)
    args_t = (RDT, *box, g.tmask_device_ptr, C.c_void_p(g.area_t_device.data_ptr()),
              *[F[k].device_ptr for k in ("un", "vn", "hu", "hv", "ht", "sshn_t", "sshn_u", "sshn_v", "ssha")], cin, cout, 1, sp)
    ys, ye, xs, xe = it.ystart - 1, it.ystop, it.xstart - 1, it.xstop
    un, vn = F["un"].data, F["vn"].data
    o_ut, o_vt, o_sp = (out[k].data[ys:ye, xs:xe] for k in (1, 2, 3))

    def torch3():
        ut = 0.5 * (un[ys:ye, xs - 1:xe - 1] + un[ys:ye, xs:xe])
        vt = 0.5 * (vn[ys - 1:ye - 1, xs:xe] + vn[ys:ye, xs:xe])
        o_ut.copy_(ut)
        o_vt.copy_(vt)
        o_sp.copy_(torch.sqrt(ut * ut + vt * vt))

    variants = {
        "set6": lambda: D._cabi.check(L.dlesm_flow_output_f64(0, 0.0, *box, *ins, p6, sp)),
        "tracer": lambda: D._cabi.check(L.dlesm_tracer_step_f64(*args_t)),
        "set3": lambda: D._cabi.check(L.dlesm_flow_output_f64(0, 0.0, *box, *ins, p3, sp)),
        "add6": lambda: D._cabi.check(L.dlesm_flow_output_f64(1, 0.25, *box, *ins, p6, sp)),
        "torch3": torch3,
    }
    launches = 40 if n <= 4096 else 12                                 # windows of tens of milliseconds
    times = {k: [] for k in variants}
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for fn in variants.values():                                   # warm-up: code objects, first touches, torch's allocator
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
    gbs = {k: BYTES[k] * cells / med[k] / 1e6 for k in BYTES}
    spread = max(times["tracer"]) / med["tracer"]
    ratio = med["set6"] / med["tracer"]
    r = {"extents": [g.nx, g.ny], "cells": cells, "launches_per_window": launches, "ms": med, "ms_all_windows": times,
         "gbs": gbs, "set6_over_tracer": ratio, "tracer_spread": spread,
         "not_longer_than_the_tracer_sweep": bool(ratio <= spread), "torch3_over_set3": med["torch3"] / med["set3"],
         "add6_over_set6": med["add6"] / med["set6"]}
    result["sizes"][str(n)] = r
    print("| N | set6, ms | GB/s (100 B/cell) | tracer sweep, ms | set6 / tracer | tracer's max / median | set3, ms | add6, ms | "
          "torch3, ms | torch3 / set3 |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    print("| %d | %.4f | %.0f | %.4f | %.3f | %.3f | %.4f | %.4f | %.4f | %.2f |" % (
        n, med["set6"], gbs["set6"], med["tracer"], ratio, spread, med["set3"], med["add6"], med["torch3"],
        med["torch3"] / med["set3"]), flush=True)
    del F, g, variants, out, un, vn, o_ut, o_vt, o_sp, torch3
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", out_path)
