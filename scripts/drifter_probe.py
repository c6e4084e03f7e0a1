"""Drifters (dlesm_drifter_step_f64) in one process, by scripts/flow_output_probe.py's method: ms per
call as medians of interleaved windows (device events around each window, every variant warmed up first; the particles are
put back to their start before each window, outside the timed span).  The flow is a closed basin of N x N wet cells, N =
4096 and 8192, with one basin-wide gyre of at most 1 m/s on a 1000 m mesh and h = 300 s, so that a substep moves a particle
at most 0.3 cells and none runs aground.  2^20 and 2^22 particles, uniformly random over the basin, once in row-major cell
order ("sorted") and once as a random permutation of the same particles ("permuted"); nsub = 1 and 4.  Timed in the same
windows on the same arrays:
  hip      one dlesm_drifter_step_f64 call
  torch    the same rule as torch expressions -- index gathers and torch.where -- what a user would otherwise write on the
           device (yardstick 1; its result is compared with the kernel's bit for bit before anything is timed)
  stream   px, py and status read and written once by three elementwise torch launches, 40 B per particle: the floor no
           gather kernel reaches (yardstick 2, context only)
  hip4x1   (with nsub = 4 only) four calls with nsub = 1
Reported: particle-substeps per second, torch / hip, sorted / permuted, the substep loop against four calls.  Writes
profiles/r21_drifter.json and prints the LAB_NOTES table.
    python scripts/drifter_probe.py [OUT.json] [WINDOWS] [N ...]"""
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch  # noqa: E402

import dl_esm_inf_amd as D  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r21_drifter.json"
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 7
sizes = [int(a) for a in sys.argv[3:]] or [4096, 8192]
COUNTS = [1 << 20, 1 << 22]
H = 300.0
torch.cuda.set_device(0)
D.parallel_init(0, 1)
L = D._cabi.lib()
s = torch.cuda.Stream()
sp = C.c_void_p(s.cuda_stream)
f64, i32 = torch.float64, torch.int32


def ptr(t):
    return C.c_void_p(t.data_ptr())


def torch_step(h, nsub, box, ld, tm, dx_t, dy_t, un, vn, px, py, st):
    """the rule of section 6.17 on flat arrays, all particles at once (tests/drifter_numpy.py's array form)"""
    xs, xe, ys, ye = box

    def inbox(x, y):
        return (x >= xs) & (x < xe + 1.0) & (y >= ys) & (y < ye + 1.0)

    def cells(ok, x, y, o0):
        o = (torch.floor(torch.where(ok, y, 1.0)).long() - 1) * ld + (torch.floor(torch.where(ok, x, 1.0)).long() - 1)
        return torch.where(ok, o, o0)

    def vel(x, y, o):
        zero = torch.zeros_like(x)
        ue, uw = torch.where(tm[o + 1] != 0, un[o], zero), torch.where(tm[o - 1] != 0, un[o - 1], zero)
        vn_, vs = torch.where(tm[o + ld] != 0, vn[o], zero), torch.where(tm[o - ld] != 0, vn[o - ld], zero)
        a, b = x - (o % ld + 1).double(), y - (o // ld + 1).double()
        return (h * (uw + (ue - uw) * a)) / dx_t[o], (h * (vs + (vn_ - vs) * b)) / dy_t[o]

    act = st == 0
    x, y, new = px.clone(), py.clone(), st.clone()
    ok = inbox(x, y)
    o = cells(ok, x, y, torch.full_like(st, (ys - 1) * ld + xs - 1, dtype=torch.long))
    t = tm[o]
    new = torch.where(act & ~ok, 1, torch.where(act & ok & (t < 0), 2, torch.where(act & ok & (t == 0), 3, new)))
    live = act & ok & (t > 0)
    for _ in range(nsub):
        k1x, k1y = vel(x, y, o)
        xm, ym = x + 0.5 * k1x, y + 0.5 * k1y
        in_m = inbox(xm, ym)
        om = cells(in_m, xm, ym, o)
        kmx, kmy = vel(torch.where(in_m, xm, x), torch.where(in_m, ym, y), om)
        mid = in_m & (tm[om] > 0)
        xn, yn = x + torch.where(mid, kmx, k1x), y + torch.where(mid, kmy, k1y)
        in_n = inbox(xn, yn)
        on = cells(in_n, xn, yn, o)
        tn = tm[on]
        left, ground, move = live & ~in_n, live & in_n & (tn == 0), live & in_n & (tn != 0)
        x, y, o = torch.where(left | move, xn, x), torch.where(left | move, yn, y), torch.where(move, on, o)
        new = torch.where(left, 1, torch.where(ground, 3, torch.where(move & (tn < 0), 2, new)))
        live = move & (tn > 0)
    px.copy_(torch.where(act, x, px))
    py.copy_(torch.where(act, y, py))
    st.copy_(torch.where(act, new, st))


result = {"what": "ms per call, medians of interleaved windows (device events around each window): hip = one "
                  "dlesm_drifter_step_f64 call, torch = the same rule as torch expressions (yardstick 1), stream = px, py and "
                  "status read and written once by three torch launches, 40 B per particle (yardstick 2, context), hip4x1 = "
                  "four calls with nsub = 1; msubsteps_per_s = particles * nsub / ms / 1000",
          "windows": windows, "device": torch.cuda.get_device_name(0), "h": H, "configs": []}
rows = []
all_faster = True
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
        # psi = sin(pi (x - 2) / N) sin(pi (y - 2) / N): un on the east faces x = i + 1, vn on the north faces y = j + 1
        un = (-torch.sin(math.pi * (ii - 1.0) / n) * torch.cos(math.pi * (jj - 1.5) / n)).contiguous()
        vn = (torch.cos(math.pi * (ii - 1.5) / n) * torch.sin(math.pi * (jj - 1.0) / n)).contiguous()
        dx_t = torch.full((ny, ld), 1000.0, dtype=f64, device="cuda")
        dy_t = torch.full((ny, ld), 1000.0, dtype=f64, device="cuda")
        flat = [t.view(-1) for t in (tm, dx_t, dy_t, un, vn)]
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

        def put(which):
            px.copy_(start[which][0])
            py.copy_(start[which][1])
            st.zero_()

        def hip(nsub):
            D._cabi.check(L.dlesm_drifter_step_f64(H, nsub, ld, ny, *box, *F, count, *P, sp))

        def stream_pass():
            px.mul_(1.0)
            py.mul_(1.0)
            st.add_(0)

        med = {}
        with torch.cuda.stream(s):
            # the torch form computes what the kernel computes: compared once, bit for bit
            put("permuted")
            hip(4)
            got = [t.clone() for t in (px, py, st)]
            put("permuted")
            torch_step(H, 4, box, ld, *flat, px, py, st)
            s.synchronize()
            same = all(torch.equal(a.view(i32), b.view(i32)) for a, b in zip(got, (px, py, st)))
            active = int((st == 0).sum().item())
            print("N", n, "particles", count, "torch form equals the kernel bit for bit:", same, "still ACTIVE:", active, flush=True)
            variants = {}
            for which in ("sorted", "permuted"):
                for nsub in (1, 4):
                    variants[("hip", which, nsub)] = (which, lambda nsub=nsub: hip(nsub))
                    variants[("torch", which, nsub)] = (which, lambda nsub=nsub: torch_step(H, nsub, box, ld, *flat, px, py, st))
                variants[("hip4x1", which, 4)] = (which, lambda: [hip(1) for _ in range(4)])
            variants[("stream", "sorted", 0)] = ("sorted", stream_pass)
            times = {k: [] for k in variants}
            for which, fn in variants.values():
                put(which)
                fn()
                fn()
            for _ in range(windows):
                for k, (which, fn) in variants.items():
                    launches = 3 if k[0] == "torch" else 10
                    put(which)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    for _ in range(launches):
                        fn()
                    e1.record(s)
                    s.synchronize()
                    times[k].append(e0.elapsed_time(e1) / launches)
            med = {k: statistics.median(v) for k, v in times.items()}
        for which in ("sorted", "permuted"):
            for nsub in (1, 4):
                hip_ms, torch_ms = med[("hip", which, nsub)], med[("torch", which, nsub)]
                r = {"N": n, "particles": count, "order": which, "nsub": nsub, "hip_ms": hip_ms, "torch_ms": torch_ms,
                     "msubsteps_per_s": count * nsub / hip_ms / 1000.0, "torch_over_hip": torch_ms / hip_ms,
                     "hip_faster_than_torch": bool(hip_ms < torch_ms), "stream_ms": med[("stream", "sorted", 0)],
                     "hip_over_stream": hip_ms / med[("stream", "sorted", 0)],
                     "sorted_over_permuted": med[("hip", "sorted", nsub)] / med[("hip", "permuted", nsub)],
                     "hip_ms_all_windows": times[("hip", which, nsub)], "torch_ms_all_windows": times[("torch", which, nsub)],
                     "torch_equals_hip_bit_for_bit": same, "active_after_check": active}
                if nsub == 4:
                    r["hip4x1_ms"] = med[("hip4x1", which, 4)]
                    r["one_call_over_four_calls"] = hip_ms / med[("hip4x1", which, 4)]
                all_faster = all_faster and r["hip_faster_than_torch"]
                result["configs"].append(r)
                rows.append("| %d | 2^%d | %s | %d | %.4f | %.0f | %.3f | %.1f | %.4f | %.2f | %s |" % (
                    n, count.bit_length() - 1, which, nsub, hip_ms, r["msubsteps_per_s"], torch_ms, r["torch_over_hip"],
                    r["stream_ms"], r["sorted_over_permuted"],
                    "%.3f" % r["one_call_over_four_calls"] if nsub == 4 else "–"))
                print(rows[-1], flush=True)
        del px, py, st, start, variants, x0, y0, xs_, ys_, perm, order
    del tm, dx_t, dy_t, un, vn, flat, F
    torch.cuda.empty_cache()

result["hip_faster_than_torch_everywhere"] = all_faster
print("| N | particles | order | nsub | hip, ms | M particle-substeps/s | torch, ms | torch / hip | stream pass, ms | "
      "sorted / permuted | one call / four calls |")
print("|---|---|---|---|---|---|---|---|---|---|---|")
print("\n".join(rows))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", out_path, "hip faster than torch everywhere:", all_faster)
