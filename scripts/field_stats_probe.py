"""Field statistics in one sweep (dlesm_field_stats_async_f64) at 4096^2, 8192^2 and 16384^2
(DL_ESM_ALIGNMENT = 64): ms per call of
  (a) dlesm_checksum_async_f64 on one field -- the yardstick: existing code, the same bytes;
  (b) the stats of one unmasked field;
  (c) the stats of three fields in one call, against three calls of (a);
  (d) the stats of one field under a mask (12 B per cell instead of 8);
  (e) what a user does without it: torch's min, max, isfinite().all(), sum and square().sum() of the same box;
as medians of interleaved windows in one process (device events around each window); ratios to (a) of the same run against the
targets of LAB_NOTES section 5.17.
    python scripts/field_stats_probe.py [OUT.json] [WINDOWS] [SIZES]       (SIZES: comma-separated, default 4096,8192,16384)"""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

import dl_esm_inf_amd as D  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r10_field_stats.json"
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 7
sizes = [int(v) for v in sys.argv[3].split(",")] if len(sys.argv) > 3 else [4096, 8192, 16384]
PEAK = 8.0e12
TARGET = {"stats1": 1.05, "stats3_vs_3_checksums": 1.0, "stats1_masked": 1.5 * 1.05}      # at 8192^2 and 16384^2
torch.cuda.set_device(0)
D.parallel_init(0, 1)
L = D._cabi.lib()
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
result = {"what": "ms per call, medians of interleaved windows (device events around each window of back-to-back calls)",
          "windows": windows, "device": torch.cuda.get_device_name(0), "alignment": 64, "peak_Bps": PEAK,
          "targets_vs_checksum": TARGET, "cases": {}}

for n in sizes:
    ld, ny = (n + 2 + 63) // 64 * 64, n + 2
    box = (2, n + 1, 2, n + 1)
    with torch.cuda.stream(s):
        g = torch.Generator(device="cuda")
        g.manual_seed(n)
        f = [torch.rand((ny, ld), dtype=torch.float64, device="cuda", generator=g) - 0.5 for _ in range(3)]
        mask = (torch.rand((ny, ld), device="cuda", generator=g) < 0.7).to(torch.int32)
        res = torch.zeros(6 * 3 + 8, dtype=torch.float64, device="cuda")
    s.synchronize()
    fp = (C.c_void_p * 3)(*[t.data_ptr() for t in f])
    mp = (C.c_void_p * 3)(mask.data_ptr(), None, None)
    boxes = (D._cabi.Region * 3)(*[D._cabi.Region(0, 0, *box) for _ in range(3)])
    pr = C.c_void_p(res.data_ptr())
    reps = max(4, min(100, int(2e9 / (n * n))))
    inner = [t[1:n + 1, 1:n + 1] for t in f]

    def checksum(k=0):
        D._cabi.check(L.dlesm_checksum_async_f64(fp[k], ld, ny, *box, pr, sp))

    def checksum3():
        for k in range(3):
            checksum(k)

    def stats(nf, masks=None):
        return lambda: D._cabi.check(L.dlesm_field_stats_async_f64(fp, masks, boxes, nf, ld, ny, pr, sp))

    def torch5():
        with torch.cuda.stream(s):
            x = inner[0]
            x.min(), x.max(), torch.isfinite(x).all(), x.sum(), x.square().sum()

    forms = {"checksum": checksum, "stats1": stats(1), "checksum_x3": checksum3, "stats3": stats(3), "stats1_masked": stats(1, mp),
             "torch_min_max_isfinite_sum_sumsq": torch5}
    times = {k: [] for k in forms}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in forms.values():                                  # warm-up (and the stream-ordered pool's first allocation)
        for _ in range(3):
            fn()
    s.synchronize()
    for w in range(windows):
        for k, fn in forms.items():
            e0.record(s)
            for _ in range(reps):
                fn()
            e1.record(s)
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / reps)
    med = {k: statistics.median(v) for k, v in times.items()}
    ratio = {"stats1": med["stats1"] / med["checksum"], "stats3_vs_3_checksums": med["stats3"] / med["checksum_x3"],
             "stats1_masked": med["stats1_masked"] / med["checksum"],
             "stats1_vs_torch": med["stats1"] / med["torch_min_max_isfinite_sum_sumsq"]}
    case = {"ld": ld, "ny": ny, "reps_per_window": reps, "ms_median": med, "ms_all": times,
            "frac_of_peak": {"checksum": 8.0 * n * n / (med["checksum"] * 1e-3) / PEAK,
                             "stats1": 8.0 * n * n / (med["stats1"] * 1e-3) / PEAK,
                             "stats3": 24.0 * n * n / (med["stats3"] * 1e-3) / PEAK,
                             "stats1_masked": 12.0 * n * n / (med["stats1_masked"] * 1e-3) / PEAK},
            "ratio": ratio}
    if n >= 8192:
        case["meets_target"] = {k: ratio[k] <= v for k, v in TARGET.items()}
    result["cases"][str(n)] = case
    print(json.dumps({"n": n, "ms": {k: round(v, 4) for k, v in med.items()}, "ratio": {k: round(v, 4) for k, v in ratio.items()},
                      "meets": case.get("meets_target")}), flush=True)
    del f, mask, inner
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(result, fh, indent=1)
print("wrote", out_path)
