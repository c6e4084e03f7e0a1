"""The one-call NEMOLite2D-class time step (dlesm_nemolite_step_f64) at 4096^2 and 8192^2, on a closed
basin and on a tidal open channel: ms per step of the one call, of the five-launch sequence it stands for (continuity,
next_sshu, next_sshv, fused momentum, and bc_open on the channel) and of the 8-read + 1-write and 6-read + 6-write stream
copies of libdlesm_lab.so on the step's own arrays, as medians of interleaved windows in one process; % of 8 TB/s at 196
(one call) and 324 (sequence) algorithmic B/cell; one call over sequence.
    python scripts/nemolite_step_probe.py [OUT.json] [WINDOWS]"""
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dl_esm_inf_amd as D  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r07_nemolite_step.json"
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 7
PEAK = 8.0e12
BYTES = {"one_call": 196, "sequence": 324, "copy_8r1w": 72, "copy_6r6w": 96}
torch.cuda.set_device(0)
os.environ["DL_ESM_ALIGNMENT"] = "64"
D.parallel_init(0, 1)
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
result = {"what": "ms per step (per copy), medians of interleaved windows (device events around each window)",
          "windows": windows, "device": torch.cuda.get_device_name(0), "bytes_per_cell": BYTES, "peak_Bps": PEAK,
          "target": "one call <= 0.80 of the sequence at 8192^2", "cases": {}}

for n in (4096, 8192):
    for basin in ("closed", "open_channel"):
        user = np.ones((n + 2, n + 2), dtype=np.int32)
        user[0, :] = user[-1, :] = 0
        user[:, 0] = user[:, -1] = 0
        if basin == "open_channel":
            user[:, 1] = user[:, n] = -1
            user[:2, :] = 0
            user[-2:, :] = 0
        g = D.grid_type(D.GO_ARAKAWA_C, (1, 1, 2), D.GO_OFFSET_NE)
        g.decompose(n, n)
        D.grid_init(g, 1000.0, 1000.0, tmask=user)
        del user
        D.psy.coriolis(g)
        T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
        names = ("ssha", "sshn_t", "sshn_u", "sshn_v", "ssha_u", "ssha_v", "un", "vn", "ua", "va", "ht", "hu", "hv")
        F = {k: D.r2d_field(g, p) for k, p in zip(names, (T, T, U, V, U, V, U, V, U, V, T, U, V))}
        for k, f in F.items():
            D.psy.hash_init(f, 90 + len(k), stream=s)
            f.data.mul_(0.01)
            if k in ("ht", "hu", "hv"):
                f.data.add_(10.0)
        for name in ("dx_t", "dy_t", "dx_u", "dy_u", "dx_v", "dy_v", "area_t", "area_u", "area_v"):
            getattr(g, name + "_device")
        ssh_bc = None
        if basin == "open_channel":
            D.psy.open_boundary(g)
            ssh_bc = D.psy.tide_ssh(0.1, 2.0 * math.pi / 43200.0, 600.0)
        prm = D.psy.momentum_params(20.0, 0.00015, 50.0, 9.80665)
        mom = [F[k] for k in ("un", "vn", "ht", "sshn_t", "hu", "sshn_u", "hv", "sshn_v", "ssha_u", "ssha_v")]
        outs = [F[k] for k in ("ssha", "ssha_u", "ssha_v", "ua", "va")]
        ins = [F[k] for k in ("un", "vn", "ht", "hu", "hv", "sshn_t", "sshn_u", "sshn_v")]

        def one_call():
            D.psy.invoke_nemolite_step(prm, *outs, *ins, ssh_bc=ssh_bc, stream=s)

        def sequence():
            D.psy.invoke_continuity(F["ssha"], F["sshn_t"], F["sshn_u"], F["sshn_v"], F["hu"], F["hv"], F["un"], F["vn"],
                                    prm.rdt, stream=s)
            D.psy.invoke_next_sshu(F["ssha_u"], F["ssha"], stream=s)
            D.psy.invoke_next_sshv(F["ssha_v"], F["ssha"], stream=s)
            D.psy.invoke_momentum(prm, F["ua"], F["va"], *mom, stream=s)
            if ssh_bc is not None:
                D.psy.invoke_bc_open(prm, ssh_bc, F["ssha"], F["ua"], F["va"], F["hu"], F["sshn_u"], F["hv"], F["sshn_v"],
                                     F["sshn_t"], stream=s)

        nc = (g.nx * g.ny) & ~1
        src8 = (C.c_void_p * 8)(*[f.device_ptr for f in ins])
        dst1 = (C.c_void_p * 1)(F["ua"].device_ptr)
        src6 = (C.c_void_p * 6)(*[f.device_ptr for f in ins[:6]])
        spare = torch.empty(g.ny * g.nx, dtype=torch.float64, device="cuda")
        dst6 = (C.c_void_p * 6)(*[f.device_ptr for f in outs] + [spare.data_ptr()])
        variants = {
            "one_call": one_call,
            "sequence": sequence,
            "copy_8r1w": lambda: D._cabi.check_lab(D._cabi.lab().dlesm_lab_stream_copy_f64(8, 1, src8, dst1, nc, 0, sp)),
            "copy_6r6w": lambda: D._cabi.check_lab(D._cabi.lab().dlesm_lab_stream_copy_f64(6, 6, src6, dst6, nc, 0, sp)),
        }
        it = F["ssha"].internal
        cells = (it.xstop - it.xstart + 1) * (it.ystop - it.ystart + 1)
        launches = 20 if n == 4096 else 10
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
        frac = {k: BYTES[k] * (nc if k.startswith("copy") else cells) / (med[k] * 1e-3) / PEAK for k in med}
        r = {"launches_per_window": launches, "cells": cells, "ms": med, "ms_all_windows": times, "frac_of_peak": frac,
             "one_call_over_sequence": med["one_call"] / med["sequence"],
             "one_call_frac_of_copy_6r6w": frac["one_call"] / frac["copy_6r6w"]}
        result["cases"][f"{n}_{basin}"] = r
        print(n, basin, json.dumps({k: round(v, 4) for k, v in med.items()}),
              "one/seq %.3f, one call %.1f %% of peak" % (r["one_call_over_sequence"], 100 * frac["one_call"]), flush=True)
        del F, mom, outs, ins, g, variants, spare
        torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", out_path)
