"""The random walk in a varying diffusivity (dlesm_random_walk_f64) beside the constant-kh step it
extends, in one process, by scripts/dispersal_probe.py's method and on its flow: ms per call as medians of interleaved
windows (device events around each window, every variant warmed up first; the particles are put back to their start before
each window, outside the timed span).  The closed basin of N x N wet cells, N = 4096 and 8192, with one gyre of at most 1 m/s
on a 1000 m mesh and h = 300 s; 2^20 and 2^22 particles, uniformly random over the basin, once in row-major cell order
("sorted") and once as a random permutation of the same particles ("permuted"); nsub = 1 and 4.  Timed in the same windows on
the same particles, id = NULL, the tick advanced by nsub from call to call:
  dispersal   one dlesm_dispersal_step_f64 call with kh = 50 m2/s (the yardstick: the existing step of the same run)
  constant    one dlesm_random_walk_f64 call with kh_t = 50 everywhere: the same paths byte for byte, so the ratio is the cost
              of five more gathers and two square roots
  varying     one dlesm_random_walk_f64 call with kh_t = 50 (1 + 0.9 sin(2 pi i / 64) sin(2 pi j / 64)) m2/s
Before anything is timed, the constant field is compared with the dispersal step bit for bit on the device.  Writes
profiles/r27_random_walk.json and prints the table.
    python scripts/random_walk_probe.py [OUT.json] [WINDOWS] [N ...]"""
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

import dl_esm_inf_amd as D  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r27_random_walk.json"
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 7
sizes = [int(a) for a in sys.argv[3:]] or [4096, 8192]
COUNTS = [1 << 20, 1 << 22]
H, KH, SEED = 300.0, 50.0, 0x622622622
LAUNCHES = 10
torch.cuda.set_device(0)
D.parallel_init(0, 1)
L = D._cabi.lib()
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
f64, i32 = torch.float64, torch.int32


def ptr(t):
    return C.c_void_p(t.data_ptr())


result = {"what": "ms per call, medians of interleaved windows (device events around each window of %d calls): dispersal = one "
                  "dlesm_dispersal_step_f64 call (kh = %g), constant = one dlesm_random_walk_f64 call with kh_t = %g everywhere "
                  "(the same bytes), varying = with kh_t = %g (1 + 0.9 sin(2 pi i / 64) sin(2 pi j / 64)); id NULL, tick advanced "
                  "by hand; the ratios are of the medians of the same run" % (LAUNCHES, KH, KH, KH),
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
        k_const = torch.full((ny, ld), KH, dtype=f64, device="cuda")
        k_vary = (KH * (1.0 + 0.9 * torch.sin(2.0 * math.pi * ii / 64.0) * torch.sin(2.0 * math.pi * jj / 64.0))).contiguous()
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
        P = [ptr(px), ptr(py), ptr(st)]
        tick = [0]

        def put(which):
            px.copy_(start[which][0])
            py.copy_(start[which][1])
            st.zero_()

        def dispersal(nsub):
            D._cabi.check(L.dlesm_dispersal_step_f64(H, nsub, KH, SEED, tick[0], None, ld, ny, *box, *F, count, None, *P, sp))
            tick[0] += nsub

        def walk(nsub, field):
            D._cabi.check(L.dlesm_random_walk_f64(H, nsub, ptr(field), SEED, tick[0], None, ld, ny, *box, *F, count, None, *P, sp))
            tick[0] += nsub

        with torch.cuda.stream(s):
            # the constant field computes what the dispersal step computes: compared once, bit for bit, before any timing
            put("permuted")
            tick[0] = 0
            dispersal(4)
            got = [t.clone() for t in (px, py, st)]
            put("permuted")
            tick[0] = 0
            walk(4, k_const)
            s.synchronize()
            same = all(torch.equal(a.view(i32), b.view(i32)) for a, b in zip(got, (px, py, st)))
            put("permuted")
            for _ in range(LAUNCHES):
                walk(4, k_vary)
            s.synchronize()
            active = int((st == 0).sum().item())
            print("N", n, "particles", count, "the constant field equals the dispersal step bit for bit:", same,
                  "ACTIVE after a window of steps in the varying field:", active, flush=True)
            if not same:
                raise SystemExit("the constant field does not give the dispersal step's bytes: nothing is timed")
            variants = {}
            for which in ("sorted", "permuted"):
                for nsub in (1, 4):
                    variants[("dispersal", which, nsub)] = (which, lambda nsub=nsub: dispersal(nsub))
                    variants[("constant", which, nsub)] = (which, lambda nsub=nsub: walk(nsub, k_const))
                    variants[("varying", which, nsub)] = (which, lambda nsub=nsub: walk(nsub, k_vary))
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
                a, b, c = (med[(v, which, nsub)] for v in ("dispersal", "constant", "varying"))
                r = {"N": n, "particles": count, "order": which, "nsub": nsub, "dispersal_ms": a, "constant_ms": b, "varying_ms": c,
                     "constant_over_dispersal": b / a, "varying_over_dispersal": c / a,
                     "msubsteps_per_s_varying": count * nsub / c / 1000.0,
                     "dispersal_ms_all_windows": times[("dispersal", which, nsub)],
                     "constant_ms_all_windows": times[("constant", which, nsub)],
                     "varying_ms_all_windows": times[("varying", which, nsub)],
                     "constant_equals_dispersal_bit_for_bit": same, "active_after_a_window": active}
                result["configs"].append(r)
                rows.append("| %d | 2^%d | %s | %d | %.4f | %.4f | %.4f | %.3f | %.3f | %.0f |" % (
                    n, count.bit_length() - 1, which, nsub, a, b, c, b / a, c / a, r["msubsteps_per_s_varying"]))
                print(rows[-1], flush=True)
        del px, py, st, start, variants, x0, y0, xs_, ys_, perm, order
    del tm, dx_t, dy_t, un, vn, k_const, k_vary, F
    torch.cuda.empty_cache()

for key in ("constant_over_dispersal", "varying_over_dispersal"):
    ratios = [r[key] for r in result["configs"]]
    result[key + "_min_max"] = [min(ratios), max(ratios)]
print("| N | particles | order | nsub | dispersal, ms | constant kh_t, ms | varying kh_t, ms | constant / dispersal | "
      "varying / dispersal | M particle-substeps/s, varying |")
print("|---|---|---|---|---|---|---|---|---|---|")
print("\n".join(rows))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", out_path, "constant / dispersal: %.3f to %.3f, varying / dispersal: %.3f to %.3f" % (
    *result["constant_over_dispersal_min_max"], *result["varying_over_dispersal_min_max"]))
