"""The Jacobi step with its residual (dlesm_stencil5_resid_f64) at 4096^2, 8192^2 and 16384^2
(DL_ESM_ALIGNMENT = 64): ms per step of the plain step (dlesm_stencil5_f64), of the residual step with each norm, and of what a
user does without it -- the plain step followed by torch's (out - in).abs().max() over the box -- all on the same arrays,
after the planning call, as medians of interleaved windows in one process (device events around each window); ratios to the
plain step against the targets of LAB_NOTES section 5.16.
    python scripts/jacobi_resid_probe.py [OUT.json] [WINDOWS] [SIZES]       (SIZES: comma-separated, default 4096,8192,16384)"""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

import dl_esm_inf_amd as D  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r09_jacobi_resid.json"
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 7
sizes = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [4096, 8192, 16384]
PEAK = 8.0e12
TARGET = {16384: 1.02, 8192: 1.03}
torch.cuda.set_device(0)
D.parallel_init(0, 1)
L = D._cabi.lib()
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
result = {"what": "ms per step, medians of interleaved windows (device events around each window of back-to-back steps)",
          "windows": windows, "device": torch.cuda.get_device_name(0), "alignment": 64, "bytes_per_cell": 16,
          "peak_Bps": PEAK, "targets": {str(k): v for k, v in TARGET.items()}, "cases": {}}

for n in sizes:
    ld, ny = (n + 2 + 63) // 64 * 64, n + 2
    box = (2, n + 1, 2, n + 1)
    with torch.cuda.stream(s):
        g = torch.Generator(device="cuda")
        g.manual_seed(n)
        a = torch.rand((ny, ld), dtype=torch.float64, device="cuda", generator=g)
        b = torch.zeros_like(a)
        res = torch.zeros(4, dtype=torch.float64, device="cuda")
    s.synchronize()
    pa, pb, pr = C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(res.data_ptr())
    D._cabi.check(L.dlesm_stencil5_autotune_f64(pa, pb, ld, ny, *box, sp))
    shape = [C.c_int() for _ in range(4)]
    D._cabi.check(L.dlesm_stencil5_planned_shape(ld, *box, *[C.byref(v) for v in shape]))
    reps = max(4, min(100, int(2e9 / (n * n))))

    def plain():
        D._cabi.check(L.dlesm_stencil5_f64(pa, pb, ld, ny, *box, sp))

    def resid(norm):
        return lambda: D._cabi.check(L.dlesm_stencil5_resid_f64(pa, pb, ld, ny, *box, norm, pr, sp))

    def plain_then_torch():
        plain()
        with torch.cuda.stream(s):
            torch.amax((b[1:n + 1, 1:n + 1] - a[1:n + 1, 1:n + 1]).abs(), dim=(0, 1), out=res[2])

    forms = {"plain": plain, "resid_max": resid(0), "resid_sumsq": resid(1), "plain_then_torch_max": plain_then_torch}
    times = {k: [] for k in forms}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for f in forms.values():                                   # warm-up (and the stream-ordered pool's first allocation)
        for _ in range(3):
            f()
    s.synchronize()
    for w in range(windows):
        for k, f in forms.items():
            e0.record(s)
            for _ in range(reps):
                f()
            e1.record(s)
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / reps)
    med = {k: statistics.median(v) for k, v in times.items()}
    case = {"ld": ld, "ny": ny, "reps_per_window": reps,
            "planned_shape": {"waves_per_group": shape[0].value, "tiles_per_row": shape[1].value,
                              "rows_per_tile": shape[2].value, "nt_stores": shape[3].value},
            "ms_median": med, "ms_all": times,
            "frac_of_peak_plain": 16.0 * n * n / (med["plain"] * 1e-3) / PEAK,
            "ratio_to_plain": {k: med[k] / med["plain"] for k in forms if k != "plain"},
            "resid_max_vs_plain_then_torch": med["resid_max"] / med["plain_then_torch_max"]}
    if n in TARGET:
        case["target"] = TARGET[n]
        case["meets_target"] = all(case["ratio_to_plain"][k] <= TARGET[n] for k in ("resid_max", "resid_sumsq"))
    result["cases"][str(n)] = case
    print(json.dumps({"n": n, "ms": {k: round(v, 4) for k, v in med.items()},
                      "ratio": {k: round(v, 4) for k, v in case["ratio_to_plain"].items()}}), flush=True)
    del a, b
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", out_path)
