"""The cell bin (dlesm_cell_bin_f64) in one process, by scripts/particle_sort_probe.py's method and on
its basin: ms per call as medians of interleaved windows (device events around each window, every variant warmed up first).
A closed basin of N x N cells, N = 4096 and 8192 -- the box of the r21 gyre; the bin reads no flow --, 2^20 and 2^22
particles with two weights each.  Timed in the same windows:
  order            one dlesm_particle_order_f64 call on the particles, uniformly random over the basin, in random order
  count_set, count_add, three_set, three_add
                   one dlesm_cell_bin_f64 call through that perm: the count alone and the count with two weighted sums,
                   DLESM_OUT_SET and DLESM_OUT_ADD
  torch_count, torch_three
                   the torch form of the same run, the yardstick: the keys as torch expressions, torch.bincount for the
                   count and index_put_(accumulate=True) for each sum (floating-point atomics: its sums differ from run to
                   run; its counts are compared with the kernel's, exactly, before anything is timed)
  fill_one, fill_three
                   dlesm_fill_f64 over the box, once and three times: 8 B per cell and output, the floor of the SET fill
  onecell_order, onecell_count_set, onecell_three_set
                   all particles in one cell: one run over every chunk, the case the chunk rule is for
  chunkcells_three_set
                   64 particles in each of count / 64 cells, in order (perm = NULL): every wave adds 63 times as in the
                   one-cell case and no run crosses a chunk, so onecell_three_set minus this is the time of the chain of
                   partials in the last pass, and this minus three_set bounds what the long adds inside the chunks cost
Writes profiles/r23_cell_bin.json and prints the DESIGN.md table.
    python scripts/cell_bin_probe.py [OUT.json] [WINDOWS] [N ...]"""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

import dl_esm_inf_amd as D  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r23_cell_bin.json"
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 7
sizes = [int(a) for a in sys.argv[3:]] or [4096, 8192]
COUNTS = [1 << 20, 1 << 22]
SET, ADD = D._cabi.OUT_SET, D._cabi.OUT_ADD
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
                  "dlesm_particle_order_f64 call; count_* = one dlesm_cell_bin_f64 call with the count alone, three_* with the "
                  "count and two weighted sums, SET and ADD; torch_* = keys as torch expressions + torch.bincount / "
                  "index_put_(accumulate=True) (the yardstick); fill_* = dlesm_fill_f64 over the box once / three times (the "
                  "floor of the SET fill); onecell_* = all particles in one cell; chunkcells_three_set = 64 particles in each "
                  "of count / 64 cells, in order",
          "windows": windows, "device": torch.cuda.get_device_name(0), "configs": []}
rows = []
for n in sizes:
    ld, ny = n + 2, n + 2
    box = (2, n + 1, 2, n + 1)
    ncells = n * n
    for count in COUNTS:
        need_order, need = C.c_longlong(), C.c_longlong()
        D._cabi.check(L.dlesm_particle_order_scratch(count, C.byref(need_order)))
        D._cabi.check(L.dlesm_cell_bin_scratch(count, 3, C.byref(need)))
        with torch.cuda.stream(s):
            g = torch.Generator(device="cuda")
            g.manual_seed(619)
            sets = {"uniform": (2.0 + n * torch.rand(count, dtype=f64, device="cuda", generator=g),
                                2.0 + n * torch.rand(count, dtype=f64, device="cuda", generator=g))}
            frac = torch.rand(count, dtype=f64, device="cuda", generator=g)
            sets["onecell"] = (2.0 + n // 2 + frac, 2.0 + n // 3 + 0.5 * frac)
            cell = torch.arange(count, device="cuda") // 64
            sets["chunkcells"] = (2.0 + (cell % n).to(f64) + frac, 2.0 + (cell // n).to(f64) + 0.5 * frac)
            st = torch.zeros(count, dtype=i32, device="cuda")
            w1 = (torch.rand(count, dtype=f64, device="cuda", generator=g) - 0.5) * 2.0 ** 30
            w2 = torch.rand(count, dtype=f64, device="cuda", generator=g) + 1.0
            perms = {k: torch.empty(count, dtype=i32, device="cuda") for k in ("uniform", "onecell")}
            nlive = torch.empty(1, dtype=i32, device="cuda")
            flag = torch.empty(1, dtype=i32, device="cuda")
            order_scratch = torch.empty(need_order.value, dtype=torch.uint8, device="cuda")
            scratch = torch.empty(need.value, dtype=torch.uint8, device="cuda")
            outs = [torch.zeros((ny, ld), dtype=f64, device="cuda") for _ in range(3)]
        po = (C.c_void_p * 3)(*[t.data_ptr() for t in outs])
        pw = (C.c_void_p * 3)(None, w1.data_ptr(), w2.data_ptr())

        def hip_order(which="uniform"):
            x, y = sets[which]
            D._cabi.check(L.dlesm_particle_order_f64(*box, count, ptr(x), ptr(y), ptr(st), ptr(perms[which]), ptr(nlive),
                                                     ptr(order_scratch), need_order.value, sp))

        def hip_bin(mode, k, which="uniform"):
            x, y = sets[which]
            pm = ptr(perms[which]) if which in perms else None
            D._cabi.check(L.dlesm_cell_bin_f64(mode, 0.5 if mode == ADD else 1.0, ld, ny, *box, count, ptr(x), ptr(y), ptr(st), pm,
                                               k, pw, po, ptr(flag), ptr(scratch), need.value, sp))

        def torch_keys(which="uniform"):
            x, y = sets[which]
            live = (st == 0) & (x >= box[0]) & (x < box[1] + 1.0) & (y >= box[2]) & (y < box[3] + 1.0)
            key = (torch.floor(y).long() - box[2]) * n + (torch.floor(x).long() - box[0])
            return torch.where(live, key, ncells)

        def torch_form(k):
            key = torch_keys()
            res = [torch.bincount(key, minlength=ncells + 1)[:ncells].to(f64)]
            for w in (w1, w2)[:k - 1]:
                res.append(torch.zeros(ncells + 1, dtype=f64, device="cuda").index_put_((key,), w, accumulate=True))
            return res

        def fill(k):
            for t in outs[:k]:
                D._cabi.check(L.dlesm_fill_f64(ptr(t), ld, ny, *box, C.c_double(0.0), sp))

        with torch.cuda.stream(s):
            hip_order(), hip_order("onecell")
            checks = {}
            for which in ("uniform", "onecell", "chunkcells"):
                hip_bin(SET, 3, which)
                s.synchronize()
                cnt = torch.bincount(torch_keys(which), minlength=ncells + 1)[:ncells].to(f64).reshape(n, n)
                checks[which] = bool(torch.equal(outs[0][1:n + 1, 1:n + 1], cnt)) and int(flag[0]) == 0 and int(outs[0].sum()) == count
            print("N", n, "particles", count, "counts equal torch.bincount, flag 0:", checks, flush=True)
            variants = {
                "order": (lambda: hip_order(), 10), "count_set": (lambda: hip_bin(SET, 1), 10),
                "count_add": (lambda: hip_bin(ADD, 1), 10), "three_set": (lambda: hip_bin(SET, 3), 10),
                "three_add": (lambda: hip_bin(ADD, 3), 10), "torch_count": (lambda: torch_form(1), 3),
                "torch_three": (lambda: torch_form(3), 3), "fill_one": (lambda: fill(1), 10), "fill_three": (lambda: fill(3), 10),
                "onecell_order": (lambda: hip_order("onecell"), 10), "onecell_count_set": (lambda: hip_bin(SET, 1, "onecell"), 3),
                "onecell_three_set": (lambda: hip_bin(SET, 3, "onecell"), 3),
                "chunkcells_three_set": (lambda: hip_bin(SET, 3, "chunkcells"), 10),
            }
            times = {k: [] for k in variants}
            for fn, _ in variants.values():
                fn()
                fn()
            for _ in range(windows):
                for k, (fn, launches) in variants.items():
                    times[k].append(timed(fn, launches))
            med = {k: statistics.median(v) for k, v in times.items()}
        r = {"N": n, "particles": count, "counts_equal_torch_bincount": checks}
        r.update({k + "_ms": v for k, v in med.items()})
        r["torch_over_hip_count"] = med["torch_count"] / med["count_set"]
        r["torch_over_hip_three"] = med["torch_three"] / med["three_set"]
        r["onecell_over_uniform_count"] = med["onecell_count_set"] / med["count_set"]
        r["onecell_over_uniform_three"] = med["onecell_three_set"] / med["three_set"]
        r["onecell_chain_of_partials_ms"] = med["onecell_three_set"] - med["chunkcells_three_set"]
        r["fill_floor_GBps"] = 8.0 * ncells * 3 / med["fill_three"] / 1e6
        r["all_windows"] = times
        result["configs"].append(r)
        rows.append("| %d | 2^%d | %.4f | %.4f | %.4f | %.4f | %.4f | %.4f | %.4f | %.4f | %.4f | %.4f | %.4f | %.4f | %.1f |" % (
            n, count.bit_length() - 1, med["order"], med["count_set"], med["count_add"], med["three_set"], med["three_add"],
            med["torch_count"], med["torch_three"], med["fill_one"], med["fill_three"], med["onecell_count_set"],
            med["onecell_three_set"], med["chunkcells_three_set"], r["onecell_over_uniform_three"]))
        print(rows[-1], flush=True)
        del sets, st, w1, w2, perms, scratch, order_scratch, outs, variants, frac, cell, cnt
        torch.cuda.empty_cache()

print("| N | particles | order | count SET | count ADD | three SET | three ADD | torch count | torch three | fill, one | "
      "fill, three | one cell, count SET | one cell, three SET | 64 per cell, three SET | one cell / uniform (three) |")
print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
print("\n".join(rows))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", out_path)
