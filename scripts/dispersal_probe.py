"""The dispersal step (dlesm_dispersal_step_f64) beside the drifter step it extends, in one process,
by scripts/drifter_probe.py's method and on its flow: ms per call as medians of interleaved windows (device events around each
window, every variant warmed up first; the particles are put back to their start before each window, outside the timed
span).  The closed basin of N x N wet cells, N = 4096 and 8192, with one gyre of at most 1 m/s on a 1000 m mesh and h = 300 s;
2^20 and 2^22 particles, uniformly random over the basin, once in row-major cell order ("sorted") and once as a random
permutation of the same particles ("permuted"); nsub = 1 and 4.  kh = 50 m2/s, an amplitude of 300 m: a kick of at most 0.3
cells per axis and substep on top of the flow's 0.3.  Timed in the same windows on the same particles:
  drifter     one dlesm_drifter_step_f64 call (the yardstick: the existing step of the same run)
  dispersal   one dlesm_dispersal_step_f64 call with id = NULL, the tick advanced by nsub from call to call
  ids         (permuted, nsub = 4 only) the same with an id array
  counter     (permuted, nsub = 4 only) the same with the device counter, whose one-lane launch follows the step
Before anything is timed, kh = 0 is compared with the drifter step bit for bit.  Over the ten calls of a window the kicks
take the "sorted" particles about a cell out of order; the drifter step's particles move along the gyre together.  Writes
profiles/r25_dispersal.json and prints the table.
    python scripts/dispersal_probe.py [OUT.json] [WINDOWS] [N ...]"""
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

import dl_esm_inf_amd as D  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r25_dispersal.json"
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 7
sizes = [int(a) for a in sys.argv[3:]] or [4096, 8192]
COUNTS = [1 << 20, 1 << 22]
H, KH, SEED = 300.0, 50.0, 0x620620620
LAUNCHES = 10
torch.cuda.set_device(0)
D.parallel_init(0, 1)
L = D._cabi.lib()
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
f64, i32 = torch.float64, torch.int32


def ptr(t):
    return C.c_void_p(t.data_ptr())


result = {"what": "ms per call, medians of interleaved windows (device events around each window of %d calls): drifter = one "
                  "dlesm_drifter_step_f64 call, dispersal = one dlesm_dispersal_step_f64 call (kh = %g, id NULL, tick advanced "
                  "by hand), ids = with an id array, counter = with the device counter and its one-lane launch; "
                  "dispersal_over_drifter = the ratio of the two medians of the same run" % (LAUNCHES, KH),
          "windows": windows, "device": torch.cuda.get_device_name(0), "h": H, "kh": KH, "configs": []}
rows = []
for n in sizes:
    ld, ny = n + 2, n + 2
    box = (2, n + 1, 2, n + 1)
    with torch.cuda.stream(s):
        g = torch.Generator(device="cuda")
        g.manual_seed(617)
        tm = torch.ones((ny, ld), dtype=i32, device="cuda")
        tm[0, :] = 0
        tm[-1, :] = 0
        tm[:, 0] = 0
        tm[:, -1] = 0
        jj = torch.arange(1, ny + 1, dtype=f64, device="cuda")[:, None]
        ii = torch.arange(1, ld + 1, dtype=f64, device="cuda")[None, :]
        un = (-torch.sin(math.pi * (ii - 1.0) / n) * torch.cos(math.pi * (jj - 1.5) / n)).contiguous()
        vn = (torch.cos(math.pi * (ii - 1.5) / n) * torch.sin(math.pi * (jj - 1.0) / n)).contiguous()
        dx_t = torch.full((ny, ld), 1000.0, dtype=f64, device="cuda")
        dy_t = torch.full((ny, ld), 1000.0, dtype=f64, device="cuda")
    F = [ptr(t) for t in (tm, dx_t, dy_t, un, vn)]
    for count in COUNTS:
        with torch.cuda.stream(s):
            x0 = 2.0 + n * torch.rand(count, dtype=f64, device="cuda", generator=g)
            y0 = 2.0 + n * torch.rand(count, dtype=f64, device="cuda", generator=g)
            order = torch.argsort(torch.floor(y0).long() * ld + torch.floor(x0).long())
            xs_, ys_ = x0[order].contiguous(), y0[order].contiguous()
            perm = torch.randperm(count, device="cuda", generator=g)
            start = {"sorted": (xs_, ys_), "permuted": (xs_[perm].contiguous(), ys_[perm].contiguous())}
            px, py = torch.empty_like(x0), torch.empty_like(y0)
            st = torch.zeros(count, dtype=i32, device="cuda")
            ids = torch.arange(count, dtype=i32, device="cuda")
            counter = torch.zeros(1, dtype=torch.int64, device="cuda")
        P = [ptr(px), ptr(py), ptr(st)]
        tick = [0]

        def put(which):
            px.copy_(start[which][0])
            py.copy_(start[which][1])
            st.zero_()

        def drifter(nsub):
            D._cabi.check(L.dlesm_drifter_step_f64(H, nsub, ld, ny, *box, *F, count, *P, sp))

        def dispersal(nsub, kh=KH, id_=None, tick_dev=None):
            D._cabi.check(L.dlesm_dispersal_step_f64(H, nsub, kh, SEED, tick[0], tick_dev, ld, ny, *box, *F, count, id_, *P, sp))
            tick[0] += nsub

        with torch.cuda.stream(s):
            # kh = 0 computes what the drifter step computes: compared once, bit for bit
            put("permuted")
            drifter(4)
            got = [t.clone() for t in (px, py, st)]
            put("permuted")
            dispersal(4, kh=0.0)
            s.synchronize()
            same = all(torch.equal(a.view(i32), b.view(i32)) for a, b in zip(got, (px, py, st)))
            put("permuted")
            for _ in range(LAUNCHES):
                dispersal(4)
            s.synchronize()
            active = int((st == 0).sum().item())
            print("N", n, "particles", count, "kh = 0 equals the drifter step bit for bit:", same,
                  "ACTIVE after a window of dispersal steps:", active, flush=True)
            variants = {}
            for which in ("sorted", "permuted"):
                for nsub in (1, 4):
                    variants[("drifter", which, nsub)] = (which, lambda nsub=nsub: drifter(nsub))
                    variants[("dispersal", which, nsub)] = (which, lambda nsub=nsub: dispersal(nsub))
            variants[("ids", "permuted", 4)] = ("permuted", lambda: dispersal(4, id_=ptr(ids)))
            variants[("counter", "permuted", 4)] = ("permuted", lambda: dispersal(4, tick_dev=ptr(counter)))
            times = {k: [] for k in variants}
            for which, fn in variants.values():
                put(which)
                fn()
                fn()
            for _ in range(windows):
                for k, (which, fn) in variants.items():
                    put(which)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for _ in range(LAUNCHES):
                        fn()
                    e1.record(s)
                    s.synchronize()
                    times[k].append(e0.elapsed_time(e1) / LAUNCHES)
            med = {k: statistics.median(v) for k, v in times.items()}
        for which in ("sorted", "permuted"):
            for nsub in (1, 4):
                a, b = med[("drifter", which, nsub)], med[("dispersal", which, nsub)]
                r = {"N": n, "particles": count, "order": which, "nsub": nsub, "drifter_ms": a, "dispersal_ms": b,
                     "dispersal_over_drifter": b / a, "msubsteps_per_s": count * nsub / b / 1000.0,
                     "drifter_ms_all_windows": times[("drifter", which, nsub)],
                     "dispersal_ms_all_windows": times[("dispersal", which, nsub)],
                     "kh_zero_equals_drifter_bit_for_bit": same, "active_after_a_window": active}
                if which == "permuted" and nsub == 4:
                    r["ids_ms"], r["counter_ms"] = med[("ids", "permuted", 4)], med[("counter", "permuted", 4)]
                result["configs"].append(r)
                rows.append("| %d | 2^%d | %s | %d | %.4f | %.4f | %.3f | %.0f | %s |" % (
                    n, count.bit_length() - 1, which, nsub, a, b, b / a, r["msubsteps_per_s"],
                    "%.4f / %.4f" % (r["ids_ms"], r["counter_ms"]) if "ids_ms" in r else "–"))
                print(rows[-1], flush=True)
        del px, py, st, start, variants, x0, y0, xs_, ys_, perm, order, ids, counter
    del tm, dx_t, dy_t, un, vn, F
    torch.cuda.empty_cache()

ratios = [r["dispersal_over_drifter"] for r in result["configs"]]
result["dispersal_over_drifter_min_max"] = [min(ratios), max(ratios)]
print("| N | particles | order | nsub | drifter, ms | dispersal, ms | dispersal / drifter | M particle-substeps/s | "
      "with ids / with the counter, ms |")
print("|---|---|---|---|---|---|---|---|---|")
print("\n".join(rows))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", out_path, "dispersal / drifter: %.3f to %.3f" % (min(ratios), max(ratios)))
