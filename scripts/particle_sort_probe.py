"""The particle order (dlesm_particle_order_f64 and dlesm_particle_permute) in one process, by
scripts/drifter_probe.py's method and on its flow: ms per call as medians of interleaved windows (device events around each
window, every variant warmed up first; the particles are put back to their start before each window, outside the timed
span).  A closed basin of N x N wet cells, N = 4096 and 8192, one gyre of at most 1 m/s on a 1000 m mesh, h = 300 s; 2^20 and
2^22 particles, uniformly random over the basin, in a random order.  Timed in the same windows:
  order        one dlesm_particle_order_f64 call on the permuted particles (perm and nlive)
  permute      one dlesm_particle_permute call of px, py and status through that perm
  torch_order  the keys as torch expressions and torch.sort(keys, stable=True): what a Python caller would otherwise write
               (the yardstick; its permutation is compared with the kernel's, exactly, before anything is timed)
  torch_gather three index gathers through the permutation
  step_permuted, step_sorted, step_argsort   dlesm_drifter_step_f64 (nsub = 1) on the permuted particles, on what order +
               permute made of them, and on the same particles in torch.argsort's cell order (profiles/r21_drifter.json's
               "sorted" row)
Then, in windows of their own: sort, then 101 steps with the step timed 0, 10, 50 and 100 steps after the sort, against the
same 101 steps without a sort.  Reported: the break-even (order + permute) / (step_permuted - step_sorted) in steps.  Writes
profiles/r22_particle_sort.json and prints the LAB_NOTES tables.
    python scripts/particle_sort_probe.py [OUT.json] [WINDOWS] [N ...]"""
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

import dl_esm_inf_amd as D  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r22_particle_sort.json"
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 7
sizes = [int(a) for a in sys.argv[3:]] or [4096, 8192]
COUNTS = [1 << 20, 1 << 22]
H = 300.0
AFTER = [0, 10, 50, 100]
torch.cuda.set_device(0)
D.parallel_init(0, 1)
L = D._cabi.lib()
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
f64, i32 = torch.float64, torch.int32


def ptr(t):
    return C.c_void_p(t.data_ptr())


def timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(launches):
        fn()
    e1.record(s)
    s.synchronize()
    return e0.elapsed_time(e1) / launches


result = {"what": "ms per call, medians of interleaved windows (device events around each window); order = one "
                  "dlesm_particle_order_f64 call, permute = one dlesm_particle_permute call of px, py, status; torch_order = "
                  "keys as torch expressions + torch.sort(stable=True), torch_gather = three index gathers (the yardstick); "
                  "step_* = dlesm_drifter_step_f64 with nsub = 1; break_even_steps = (order + permute) / (step_permuted - "
                  "step_sorted); after_sort_ms = the step 0, 10, 50, 100 steps after a sort, no_sort_ms = the same steps of "
                  "the same run without one",
          "windows": windows, "device": torch.cuda.get_device_name(0), "h": H, "configs": []}
rows, drift_rows = [], []
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
        need = C.c_longlong()
        D._cabi.check(L.dlesm_particle_order_scratch(count, C.byref(need)))
        with torch.cuda.stream(s):
            x0 = 2.0 + n * torch.rand(count, dtype=f64, device="cuda", generator=g)
            y0 = 2.0 + n * torch.rand(count, dtype=f64, device="cuda", generator=g)
            order = torch.argsort(torch.floor(y0).long() * ld + torch.floor(x0).long())
            xs_, ys_ = x0[order].contiguous(), y0[order].contiguous()
            shuffle = torch.randperm(count, device="cuda", generator=g)
            start = {"argsort": (xs_, ys_), "permuted": (xs_[shuffle].contiguous(), ys_[shuffle].contiguous())}
            px, py = torch.empty_like(x0), torch.empty_like(y0)
            st = torch.zeros(count, dtype=i32, device="cuda")
            qx, qy, qs = torch.empty_like(px), torch.empty_like(py), torch.empty_like(st)
            perm = torch.empty(count, dtype=i32, device="cuda")
            nlive = torch.empty(1, dtype=i32, device="cuda")
            scratch = torch.empty(need.value, dtype=torch.uint8, device="cuda")
        P, Q = [ptr(px), ptr(py), ptr(st)], [ptr(qx), ptr(qy), ptr(qs)]
        src, dst = (C.c_void_p * 3)(*[t.data_ptr() for t in (px, py, st)]), (C.c_void_p * 3)(*[t.data_ptr() for t in (qx, qy, qs)])
        eb = (C.c_int * 3)(8, 8, 4)

        def put(which):
            px.copy_(start[which][0])
            py.copy_(start[which][1])
            st.zero_()

        def hip_order():
            D._cabi.check(L.dlesm_particle_order_f64(*box, count, *P, ptr(perm), ptr(nlive), ptr(scratch), need.value, sp))

        def hip_permute():
            D._cabi.check(L.dlesm_particle_permute(count, ptr(perm), 3, src, dst, eb, sp))

        def torch_keys():
            live = (st == 0) & (px >= box[0]) & (px < box[1] + 1.0) & (py >= box[2]) & (py < box[3] + 1.0)
            key = (torch.floor(py).to(i32) - box[2]) * n + (torch.floor(px).to(i32) - box[0])
            return torch.where(live, key, n * n)

        def torch_order():
            return torch.sort(torch_keys(), stable=True)[1]

        def step(arrays=P):
            D._cabi.check(L.dlesm_drifter_step_f64(H, 1, ld, ny, *box, *F, count, *arrays, sp))

        with torch.cuda.stream(s):
            put("permuted")
            hip_order()
            tperm = torch_order()
            s.synchronize()
            same = bool(torch.equal(perm.long(), tperm)) and int(nlive[0]) == count
            print("N", n, "particles", count, "perm equals torch.sort(stable=True):", same, flush=True)
            hip_permute()
            sorted_start = (qx.clone(), qy.clone())
            start["sorted"] = sorted_start
            state = {"tperm": tperm}

            def torch_gather():
                t = state["tperm"]
                return px[t], py[t], st[t]

            variants = {
                "order": ("permuted", hip_order, 10), "permute": ("permuted", hip_permute, 10),
                "torch_order": ("permuted", torch_order, 3), "torch_gather": ("permuted", torch_gather, 10),
                "step_permuted": ("permuted", step, 10), "step_sorted": ("sorted", step, 10),
                "step_argsort": ("argsort", step, 10),
            }
            times = {k: [] for k in variants}
            for which, fn, _ in variants.values():
                put(which)
                fn()
                fn()
            for _ in range(windows):
                for k, (which, fn, launches) in variants.items():
                    put(which)
                    times[k].append(timed(fn, launches))
            med = {k: statistics.median(v) for k, v in times.items()}

            # how the gain decays: the step 0, 10, 50, 100 steps after a sort, against the same steps without one
            after = {k: [] for k in AFTER}
            plain = {k: [] for k in AFTER}
            for _ in range(windows):
                for sort_first, into in ((True, after), (False, plain)):
                    put("permuted")
                    if sort_first:
                        hip_order()
                        hip_permute()
                        px.copy_(qx), py.copy_(qy), st.copy_(qs)
                    for k in range(AFTER[-1] + 1):
                        if k in into:
                            into[k].append(timed(step, 1))
                        else:
                            step()
            after_med = {k: statistics.median(v) for k, v in after.items()}
            plain_med = {k: statistics.median(v) for k, v in plain.items()}
        gain = med["step_permuted"] - med["step_sorted"]
        r = {"N": n, "particles": count, "perm_equals_torch_stable_sort": same, "passes": (int(n * n).bit_length() + 7) // 8,
             "order_ms": med["order"], "permute_ms": med["permute"], "torch_order_ms": med["torch_order"],
             "torch_gather_ms": med["torch_gather"],
             "torch_over_hip": (med["torch_order"] + med["torch_gather"]) / (med["order"] + med["permute"]),
             "step_permuted_ms": med["step_permuted"], "step_sorted_ms": med["step_sorted"],
             "step_argsort_ms": med["step_argsort"], "break_even_steps": (med["order"] + med["permute"]) / gain,
             "after_sort_ms": {str(k): v for k, v in after_med.items()}, "no_sort_ms": {str(k): v for k, v in plain_med.items()},
             "all_windows": {k: v for k, v in times.items()}}
        result["configs"].append(r)
        rows.append("| %d | 2^%d | %.4f | %.4f | %.4f | %.4f | %.2f | %.4f | %.4f | %.4f | %.1f |" % (
            n, count.bit_length() - 1, r["order_ms"], r["permute_ms"], r["torch_order_ms"], r["torch_gather_ms"],
            r["torch_over_hip"], r["step_permuted_ms"], r["step_sorted_ms"], r["step_argsort_ms"], r["break_even_steps"]))
        drift_rows.append("| %d | 2^%d | %s | %s |" % (n, count.bit_length() - 1,
                                                      " | ".join("%.4f" % after_med[k] for k in AFTER),
                                                      " | ".join("%.4f" % plain_med[k] for k in AFTER)))
        print(rows[-1], flush=True)
        print(drift_rows[-1], flush=True)
        del px, py, st, qx, qy, qs, perm, scratch, start, variants, x0, y0, xs_, ys_, shuffle, order, tperm, state, sorted_start
    del tm, dx_t, dy_t, un, vn, F
    torch.cuda.empty_cache()

print("| N | particles | order, ms | permute, ms | torch keys + sort, ms | torch gathers, ms | torch / hip | step permuted, ms | "
      "step after the sort, ms | step in argsort order, ms | break-even, steps |")
print("|---|---|---|---|---|---|---|---|---|---|---|")
print("\n".join(rows))
print("| N | particles | " + " | ".join("%d after a sort, ms" % k for k in AFTER) + " | " +
      " | ".join("%d without, ms" % k for k in AFTER) + " |")
print("|---|---|" + "---|" * (2 * len(AFTER)))
print("\n".join(drift_rows))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", out_path)
