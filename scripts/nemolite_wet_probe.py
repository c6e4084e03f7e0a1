"""The NEMOLite2D-class time step that skips land (dlesm_nemolite_step_wet_f64) at 8192^2, in one
process: ms per step of the existing entry (dlesm_nemolite_step_f64, the reference) and of the wet entry in both forms of its
kernel -- the flag map (nemo_wet_form = 0) and the compacted list (nemo_wet_form = 1) -- as medians of interleaved windows,
on four masks: all wet, one land block over half the box, a checkerboard of 512 x 512 land and sea squares, and a ragged
coast (a thresholded smooth random field, about 40 % land).  Beside each time ratio the plan's active / tiles: a step that
does no work on inactive tiles should cost about that share of the full step.
    python scripts/nemolite_wet_probe.py [OUT.json] [WINDOWS] [N]"""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dl_esm_inf_amd as D  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r09_nemolite_wet.json"
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 7
n = int(sys.argv[3]) if len(sys.argv) > 3 else 8192
torch.cuda.set_device(0)
os.environ["DL_ESM_ALIGNMENT"] = "64"
D.parallel_init(0, 1)
L = D._cabi.lib()
s = torch.cuda.Stream()
result = {"what": "ms per step, medians of interleaved windows (device events around each window); full = "
                  "dlesm_nemolite_step_f64, flags / list = dlesm_nemolite_step_wet_f64 with nemo_wet_form = 0 / 1",
          "n": n, "windows": windows, "device": torch.cuda.get_device_name(0),
          "yardstick": "time ratio against active / tiles", "cases": {}}


def masks():
    m = np.ones((n + 2, n + 2), dtype=np.int32)
    yield "all_wet", m
    m = np.ones((n + 2, n + 2), dtype=np.int32)
    m[1:n + 1, 1:n // 2 + 1] = 0
    yield "half_block", m
    jj, ii = np.mgrid[0:n + 2, 0:n + 2]
    yield "checker_512", (((ii // 512) + (jj // 512)) % 2).astype(np.int32)
    gen = torch.Generator().manual_seed(40)
    coarse = torch.randn((1, 1, 33, 33), generator=gen, dtype=torch.float64)
    smooth = torch.nn.functional.interpolate(coarse, size=(n + 2, n + 2), mode="bicubic", align_corners=True)[0, 0].numpy()
    yield "ragged_coast", (smooth > np.quantile(smooth, 0.4)).astype(np.int32)


for name, user in masks():
    user[0, :] = user[-1, :] = 0
    user[:, 0] = user[:, -1] = 0
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
    for m in ("dx_t", "dy_t", "dx_u", "dy_u", "dx_v", "dy_v", "area_t", "area_u", "area_v"):
        getattr(g, m + "_device")
    it = F["ssha"].internal
    land = float((g.tmask[it.ystart - 1:it.ystop, it.xstart - 1:it.xstop] == 0).mean())
    plan = D.psy.wet_plan(g)
    prm = D.psy.momentum_params(20.0, 0.00015, 50.0, 9.80665)
    outs = [F[k] for k in ("ssha", "ssha_u", "ssha_v", "ua", "va")]
    ins = [F[k] for k in ("un", "vn", "ht", "hu", "hv", "sshn_t", "sshn_u", "sshn_v")]

    def full():
        D.psy.invoke_nemolite_step(prm, *outs, *ins, stream=s)

    def wet(form):
        def fn():
            L.dlesm_set_tuning(b"nemo_wet_form", form)
            D.psy.invoke_nemolite_step(prm, *outs, *ins, stream=s, skip_land=True)
        return fn

    variants = {"full": full, "flags": wet(0), "list": wet(1)}
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
    L.dlesm_set_tuning(b"nemo_wet_form", 0)
    med = {k: statistics.median(v) for k, v in times.items()}
    share = plan.active / plan.tiles
    r = {"land_share_of_cells": land, "tiles": plan.tiles, "active": plan.active, "active_over_tiles": share, "ms": med,
         "ms_all_windows": times, "flags_over_full": med["flags"] / med["full"], "list_over_full": med["list"] / med["full"]}
    result["cases"][name] = r
    print(name, "land %.3f active/tiles %.3f" % (land, share), json.dumps({k: round(v, 4) for k, v in med.items()}),
          "flags/full %.3f list/full %.3f" % (r["flags_over_full"], r["list_over_full"]), flush=True)
    del F, outs, ins, g, variants, plan
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", out_path)
