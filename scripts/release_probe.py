"""The particle release (dlesm_release_f64) in one process, by scripts/drifter_probe.py's method: ms per
call as medians of interleaved windows (device events around each window, every variant warmed up first).  A closed basin of
4096 x 4096 wet cells; sets of 2^20 and 2^22 slots; two scenarios:
  reefs   256 sources x 16 particles a call (patches of 40 x 40 cells) into a set that is 90 % full, the FREE slots at random;
          a window is 10 calls
  spill   one source of 2^20 particles a call (a patch of 2000 x 2000 cells) into an empty set; a window is as many calls as
          the set takes (1 and 4)
Every candidate is in the box and on water, so every call stores what it asks for.  status is restored before every window,
outside the timed span.  Timed in the same windows:
  release   dlesm_release_f64
  torch     the same rule as torch expressions: a generated batch (torch.rand in place of Philox, so not the same bits), the
            owner test, the mask gather, nonzero of the accepted and of FREE, index_put_ of px, py, status and id
  unpack    dlesm_migrate_unpack_f64 at the same n filling the same number of arrivals from one message: the existing entry
            that does the slot half of the work
Writes profiles/r28_particle_release.json and prints the table.
    python scripts/release_probe.py [OUT.json] [WINDOWS]"""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

import dl_esm_inf_amd as D  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r28_particle_release.json"
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 7
N, SLOTS, SEED = 4096, [1 << 20, 1 << 22], 0x9E3779B97F4A7C15 - (1 << 64)
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
    g.manual_seed(623)
    tm = torch.ones((ny, ld), dtype=i32, device="cuda")
    tm[0, :] = 0
    tm[-1, :] = 0
    tm[:, 0] = 0
    tm[:, -1] = 0
    tmf = tm.view(-1)


def scenario(name, slots):
    if name == "reefs":
        ns, count, r = 256, 16, 20.0
        x = 100.0 + (N - 200.0) * torch.rand(ns, dtype=f64, device="cuda", generator=g)
        y = 100.0 + (N - 200.0) * torch.rand(ns, dtype=f64, device="cuda", generator=g)
        st0 = torch.where(torch.rand(slots, device="cuda", generator=g) < 0.1, FREE, ACTIVE).to(i32)
        calls = 10
    else:
        ns, count, r = 1, 1 << 20, 1000.0
        x = torch.full((1,), 0.5 * N + 2.0, dtype=f64, device="cuda")
        y = x.clone()
        st0 = torch.full((slots,), FREE, dtype=i32, device="cuda")
        calls = slots >> 20
    src = D.release_sources(x.cpu().numpy(), y.cpu().numpy(), r, r, [k << 32 for k in range(ns)], count=count)
    return ns, count, r, x, y, st0, src, calls


result = {"what": "ms per call, medians of interleaved windows (device events around each window) on a 4096^2 basin: release = "
                  "dlesm_release_f64, torch = the same rule as torch expressions (rand batch, owner test, mask gather, nonzero, "
                  "index_put_), unpack = dlesm_migrate_unpack_f64 at the same n filling as many arrivals from one message; reefs = "
                  "256 sources x 16 a call into a set 90 % full (windows of 10 calls), spill = one source of 2^20 a call into an "
                  "empty set (windows of slots / 2^20 calls); status restored before every window",
          "windows": windows, "device": torch.cuda.get_device_name(0), "configs": []}
rows = []
for slots in SLOTS:
    for name in ("reefs", "spill"):
        with torch.cuda.stream(s):
            ns, count, r, sx, sy, st0, src, calls = scenario(name, slots)
            per_call = ns * count
            px, py = torch.zeros(slots, dtype=f64, device="cuda"), torch.zeros(slots, dtype=f64, device="cuda")
            st, ids = st0.clone(), torch.zeros(slots, dtype=i64, device="cuda")
            counts = torch.zeros(16, dtype=i32, device="cuda")
            need, mneed, mbytes = C.c_longlong(), C.c_longlong(), C.c_longlong()
            D._cabi.check(L.dlesm_release_scratch(slots, ns, count, C.byref(need)))
            D._cabi.check(L.dlesm_migrate_scratch(slots, C.byref(mneed)))
            D._cabi.check(L.dlesm_migrate_bytes(per_call, 0, C.byref(mbytes)))
            scratch = torch.empty(max(need.value, mneed.value, 16), dtype=torch.uint8, device="cuda")
            msg = [torch.zeros(mbytes.value // 8, dtype=i64, device="cuda") for _ in range(2)]
            msg[0][0] = per_call
            msg[0][2:2 + 2 * per_call] = (100.0 + 1000.0 * torch.rand(2 * per_call, dtype=f64, device="cuda", generator=g)).view(i64)
            mcounts = torch.zeros(16, dtype=i32, device="cuda")
            next_id = torch.zeros((), dtype=i64, device="cuda")

        def release():
            D._cabi.check(L.dlesm_release_f64(ld, ny, *box, 0, 0, ptr(tm), ptr(src), ns, count, SEED, 0, None, slots, ptr(px), ptr(py),
                                              ptr(st), ptr(ids), None, None, ptr(counts), ptr(scratch), need.value, sp))

        def torch_release():
            """the rule as torch expressions, in place; returns the number stored"""
            u = torch.rand((2, ns, count), dtype=f64, device="cuda", generator=g) * 2.0 - 1.0
            gx, gy = (sx[:, None] + r * u[0]).view(-1), (sy[:, None] + r * u[1]).view(-1)
            owned = (gx >= box[0]) & (gx < box[1] + 1.0) & (gy >= box[2]) & (gy < box[3] + 1.0)
            cell = (torch.floor(gy).long().clamp(1, ny) - 1) * ld + (torch.floor(gx).long().clamp(1, ld) - 1)
            acc = torch.nonzero(owned & (tmf[cell] != 0)).squeeze(1)
            take = torch.nonzero(st == FREE).squeeze(1)[:acc.numel()]
            acc = acc[:take.numel()]
            px.index_put_((take,), gx[acc])
            py.index_put_((take,), gy[acc])
            ids.index_put_((take,), next_id + acc)
            st.index_put_((take,), torch.zeros(take.numel(), dtype=i32, device="cuda"))
            next_id.add_(per_call)
            return take.numel()

        def unpack():
            recv = (C.c_void_p * 2)(msg[0].data_ptr(), msg[1].data_ptr())
            D._cabi.check(L.dlesm_migrate_unpack_f64(0, *box, slots, ptr(px), ptr(py), ptr(st), ptr(ids), None, 0, per_call, recv,
                                                     ptr(mcounts), ptr(scratch), mneed.value, sp))

        with torch.cuda.stream(s):
            release()
            s.synchronize()
            rec = D._cabi.ReleaseCounts.from_buffer_copy(counts.cpu().numpy().tobytes())
            st.copy_(st0)
            stored = torch_release()
            st.copy_(st0)
            unpack()
            s.synchronize()
            arrived = int(mcounts[8].item())
            variants = {"release": release, "torch": torch_release, "unpack": unpack}
            times = {k: [] for k in variants}
            for fn in variants.values():
                st.copy_(st0)
                fn()
            for w in range(windows):
                for k, fn in variants.items():
                    st.copy_(st0)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for _ in range(calls):
                        fn()
                    e1.record(s)
                    s.synchronize()
                    times[k].append(e0.elapsed_time(e1) / calls)
            med = {k: statistics.median(v) for k, v in times.items()}
            last = D._cabi.ReleaseCounts.from_buffer_copy(counts.cpu().numpy().tobytes())
        cfg = {"slots": slots, "scenario": name, "sources": ns, "count": count, "calls_per_window": calls,
               "first_call": {"requested": rec.requested, "released": rec.released, "dropped": rec.dropped, "foreign": rec.foreign,
                              "on_land": rec.on_land},
               "torch_stored": stored, "unpack_arrived": arrived, "dropped_in_the_last_call": last.dropped,
               "all_three_store_the_same_number": rec.released == stored == arrived == per_call,
               **{k + "_ms": v for k, v in med.items()}, "release_over_torch": med["release"] / med["torch"],
               "release_over_unpack": med["release"] / med["unpack"], "all_windows_ms": times}
        result["configs"].append(cfg)
        rows.append("| 2^%d | %s | %d x %d | %.4f | %.4f | %.4f | %.3f | %.2f | %s |" % (
            slots.bit_length() - 1, name, ns, count, med["release"], med["torch"], med["unpack"], cfg["release_over_torch"],
            cfg["release_over_unpack"], cfg["all_three_store_the_same_number"]))
        print(rows[-1], flush=True)
        del px, py, st, ids, st0, scratch, msg
        torch.cuda.empty_cache()

print("| slots | scenario | sources x count | release, ms | torch, ms | unpack, ms | release / torch | release / unpack | same number stored |")
print("|---|---|---|---|---|---|---|---|---|")
print("\n".join(rows))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", out_path)
