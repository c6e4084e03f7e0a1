"""The particle migration's device work (dlesm_migrate_pack_f64 + dlesm_migrate_unpack_f64) in one
process, by scripts/drifter_probe.py's method: ms per call as medians of interleaved windows (device events around each window
of 10 calls, every variant warmed up first).  The closed basin of 4096 x 4096 wet cells with drifter_probe.py's gyre on a 1000 m
mesh; 2^20 and 2^22 slots in random order of which 0.1 %, 1 % and 10 % are LEFT just outside the box, a quarter on each side,
everything else ACTIVE inside.  The messages a neighbour would send are the rank's own, swapped, with shifts of 0: what left
west arrives "from the east" at the same place outside the box, is stored as LEFT and leaves again with the next call, so every
call of a window does the same work -- that many departures packed and that many arrivals filled -- without a restore inside
the timed span.  cap = slots / 8.  Timed in the same windows:
  one_axis    pack X + unpack X (eight launches: count, scan, scatter, twice)
  both_axes   pack X, unpack X, pack Y, unpack Y: the device work of one dlesm_migrate_f64 call without its transport
  torch       the rule of one axis as torch expressions: masks, nonzero, index gathers into messages, index scatters of the
              arrivals into the first FREE slots (compared with the kernels' arrays once, exactly, before anything is timed)
  stream      one pass over px, py, status and id: four torch sums (28 bytes a slot read once)
  drifter     one dlesm_drifter_step_f64(nsub = 1) call on the same slots
The transport between ranks is functional only and is not timed.  Writes profiles/r26_particle_migrate.json and prints the
table.
    python scripts/particle_migrate_probe.py [OUT.json] [WINDOWS]"""
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

import dl_esm_inf_amd as D  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r26_particle_migrate.json"
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 7
N, COUNTS, FRACTIONS, H, LAUNCHES = 4096, [1 << 20, 1 << 22], [0.001, 0.01, 0.1], 300.0, 10
ACTIVE, LEFT, FREE = 0, 1, 4
torch.cuda.set_device(0)
D.parallel_init(0, 1)
L = D._cabi.lib()
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
f64, i32, i64 = torch.float64, torch.int32, torch.int64


def ptr(t):
    return C.c_void_p(t.data_ptr())


ld, ny = N + 2, N + 2
box = (2, N + 1, 2, N + 1)
with torch.cuda.stream(s):
    g = torch.Generator(device="cuda")
    g.manual_seed(621)
    tm = torch.ones((ny, ld), dtype=i32, device="cuda")
    tm[0, :] = 0
    tm[-1, :] = 0
    tm[:, 0] = 0
    tm[:, -1] = 0
    jj = torch.arange(1, ny + 1, dtype=f64, device="cuda")[:, None]
    ii = torch.arange(1, ld + 1, dtype=f64, device="cuda")[None, :]
    un = (-torch.sin(math.pi * (ii - 1.0) / N) * torch.cos(math.pi * (jj - 1.5) / N)).contiguous()
    vn = (torch.cos(math.pi * (ii - 1.5) / N) * torch.sin(math.pi * (jj - 1.0) / N)).contiguous()
    dx_t = torch.full((ny, ld), 1000.0, dtype=f64, device="cuda")
    dy_t = torch.full((ny, ld), 1000.0, dtype=f64, device="cuda")
F = [ptr(t) for t in (tm, dx_t, dy_t, un, vn)]

result = {"what": "ms per call, medians of interleaved windows (device events around each window of %d calls) on a 4096^2 basin: "
                  "one_axis = dlesm_migrate_pack_f64 + dlesm_migrate_unpack_f64 for axis X, both_axes = the same for X and then Y "
                  "(the device work of one dlesm_migrate_f64 call), torch = one axis as torch expressions, stream = four torch sums "
                  "over px, py, status and id, drifter = one dlesm_drifter_step_f64(nsub = 1) call on the same slots; `leaving` of "
                  "the slots are LEFT outside the box, a quarter on each side, and arrive again where they left (shifts 0), so "
                  "every call packs and fills that many" % LAUNCHES,
          "windows": windows, "device": torch.cuda.get_device_name(0), "configs": []}
rows = []
for count in COUNTS:
    cap = count // 8
    nbytes, need = C.c_longlong(), C.c_longlong()
    D._cabi.check(L.dlesm_migrate_bytes(cap, 0, C.byref(nbytes)))
    D._cabi.check(L.dlesm_migrate_scratch(count, C.byref(need)))
    for frac in FRACTIONS:
        with torch.cuda.stream(s):
            x0 = 2.0 + N * torch.rand(count, dtype=f64, device="cuda", generator=g)
            y0 = 2.0 + N * torch.rand(count, dtype=f64, device="cuda", generator=g)
            st0 = torch.zeros(count, dtype=i32, device="cuda")
            out = torch.rand(count, device="cuda", generator=g) < frac
            side = torch.randint(0, 4, (count,), device="cuda", generator=g)
            x0 = torch.where(out & (side == 0), torch.full_like(x0, 1.5), x0)
            x0 = torch.where(out & (side == 1), torch.full_like(x0, N + 2.5), x0)
            y0 = torch.where(out & (side == 2), torch.full_like(y0, 1.5), y0)
            y0 = torch.where(out & (side == 3), torch.full_like(y0, N + 2.5), y0)
            st0[out] = LEFT
            id0 = torch.arange(count, dtype=i64, device="cuda")
            px, py, st, ids = x0.clone(), y0.clone(), st0.clone(), id0.clone()
            msgs = [torch.zeros(nbytes.value, dtype=torch.uint8, device="cuda") for _ in range(4)]
            counts = torch.zeros(16, dtype=i32, device="cuda")
            scratch = torch.empty(max(need.value, 16), dtype=torch.uint8, device="cuda")
        P = [ptr(px), ptr(py), ptr(st), ptr(ids)]
        two, zero2 = (C.c_int * 2)(1, 1), (C.c_int * 2)(0, 0)

        def phase(axis):
            send = (C.c_void_p * 2)(msgs[2 * axis].data_ptr(), msgs[2 * axis + 1].data_ptr())
            recv = (C.c_void_p * 2)(msgs[2 * axis + 1].data_ptr(), msgs[2 * axis].data_ptr())
            D._cabi.check(L.dlesm_migrate_pack_f64(axis, *box, count, *P, None, 0, two, zero2, zero2, cap, send, ptr(counts),
                                                   ptr(scratch), need.value, sp))
            D._cabi.check(L.dlesm_migrate_unpack_f64(axis, *box, count, *P, None, 0, cap, recv, ptr(counts), ptr(scratch),
                                                     need.value, sp))

        def torch_axis(tx, ty, ts, ti):
            """axis X by torch expressions, in place; returns (sent W, sent E)"""
            cand = (ts == LEFT) & torch.isfinite(tx) & torch.isfinite(ty)
            sel = [torch.nonzero(cand & (tx < box[0])).squeeze(1)[:cap], torch.nonzero(cand & (tx >= box[1] + 1.0)).squeeze(1)[:cap]]
            mx, my, mi = [tx[k] + 0.0 for k in sel], [ty[k] + 0.0 for k in sel], [ti[k] for k in sel]
            for k in sel:
                ts[k] = FREE
            ax, ay, ai = torch.cat([mx[1], mx[0]]), torch.cat([my[1], my[0]]), torch.cat([mi[1], mi[0]])     # from W: what went E
            take = torch.nonzero(ts == FREE).squeeze(1)[:ax.numel()]
            ax, ay, ai = ax[:take.numel()], ay[:take.numel()], ai[:take.numel()]
            tx[take], ty[take], ti[take] = ax, ay, ai
            inb = (ax >= box[0]) & (ax < box[1] + 1.0) & (ay >= box[2]) & (ay < box[3] + 1.0)
            ts[take] = torch.where(inb, ACTIVE, LEFT).to(i32)
            return sel[0].numel(), sel[1].numel()

        def stream_pass():
            return px.sum(), py.sum(), st.sum(), ids.sum()

        def drifter():
            D._cabi.check(L.dlesm_drifter_step_f64(H, 1, ld, ny, *box, *F, count, ptr(px), ptr(py), ptr(st), sp))

        with torch.cuda.stream(s):
            tx, ty, ts, ti = x0.clone(), y0.clone(), st0.clone(), id0.clone()
            phase(0)
            sent = torch_axis(tx, ty, ts, ti)
            s.synchronize()
            same = all(torch.equal(a, b) for a, b in zip((px, py, st, ids), (tx, ty, ts, ti)))
            rec = counts.cpu().tolist()
            variants = {"one_axis": lambda: phase(0), "both_axes": lambda: (phase(0), phase(1)),
                        "torch": lambda: torch_axis(tx, ty, ts, ti), "stream": stream_pass, "drifter": drifter}
            times = {k: [] for k in variants}
            for fn in variants.values():
                fn()
                fn()
            for w in range(windows):
                for k, fn in variants.items():
                    if k == "torch" and w >= 3:
                        continue
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for _ in range(LAUNCHES):
                        fn()
                    e1.record(s)
                    s.synchronize()
                    times[k].append(e0.elapsed_time(e1) / LAUNCHES)
            med = {k: statistics.median(v) for k, v in times.items()}
            left_now = int((st == LEFT).sum().item())
        r = {"slots": count, "leaving": frac, "cap": cap, "left_at_start": int(out.sum().item()), "left_after_the_windows": left_now,
             "first_call_sent_W_E": rec[0:2], "torch_equals_the_kernels_exactly": same and tuple(rec[0:2]) == sent,
             **{k + "_ms": v for k, v in med.items()}, "one_axis_over_drifter": med["one_axis"] / med["drifter"],
             "both_axes_over_drifter": med["both_axes"] / med["drifter"], "one_axis_over_torch": med["one_axis"] / med["torch"],
             "one_axis_over_stream": med["one_axis"] / med["stream"], "all_windows_ms": times}
        result["configs"].append(r)
        rows.append("| 2^%d | %g %% | %.4f | %.4f | %.4f | %.4f | %.4f | %.3f | %.3f | %.3f | %s |" % (
            count.bit_length() - 1, 100 * frac, med["one_axis"], med["both_axes"], med["torch"], med["stream"], med["drifter"],
            r["one_axis_over_drifter"], r["both_axes_over_drifter"], r["one_axis_over_torch"], r["torch_equals_the_kernels_exactly"]))
        print(rows[-1], flush=True)
        del px, py, st, ids, tx, ty, ts, ti, msgs, x0, y0, st0, id0, out, side
        torch.cuda.empty_cache()

print("| slots | leaving | one axis, ms | both axes, ms | torch (one axis), ms | stream, ms | drifter step, ms | one axis / drifter "
      "| both axes / drifter | one axis / torch | torch == kernels |")
print("|---|---|---|---|---|---|---|---|---|---|---|")
print("\n".join(rows))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", out_path)
