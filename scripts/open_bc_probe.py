"""Open-boundary kernels at 1024^2, 4096^2 and 8192^2 on an open channel (open first and last internal
columns, land rows north and south): ms per launch of bc_open (all three lists in one launch), of bc_ssh + flather_u +
flather_v as three launches, of one fused momentum sweep, and of the whole open-channel step (continuity, next_sshu,
next_sshv, fused momentum, bc_open), as medians of interleaved windows; bc_open's share of the step and its ratio to the
momentum sweep.
    python scripts/open_bc_probe.py [OUT.json] [WINDOWS]"""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dl_esm_inf_amd as D  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else "profiles/r06_open_bc.json"
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 7
torch.cuda.set_device(0)
os.environ["DL_ESM_ALIGNMENT"] = "64"
D.parallel_init(0, 1)
s = torch.cuda.Stream()
result = {"what": "ms per launch (per step for 'step'), medians of interleaved windows (device events around each window)",
          "windows": windows, "device": torch.cuda.get_device_name(0), "sizes": {}}

for n in (1024, 4096, 8192):
    user = np.ones((n + 2, n + 2), dtype=np.int32)
    user[:, 0] = user[:, -1] = 0
    user[:, 1] = user[:, n] = -1
    user[:2, :] = 0
    user[-2:, :] = 0
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
    for name in ("dx_t", "dy_t", "dx_u", "dy_u", "dx_v", "dy_v", "area_t", "area_u", "area_v"):
        getattr(g, name + "_device")
    plan = D.psy.open_boundary(g)
    prm = D.psy.momentum_params(20.0, 0.00015, 50.0, 9.80665)
    ssh_bc = D.psy.tide_ssh(0.1, 2.0 * math.pi / 43200.0, 600.0)
    mom = [F[k] for k in ("un", "vn", "ht", "sshn_t", "hu", "sshn_u", "hv", "sshn_v", "ssha_u", "ssha_v")]
    bc = (F["hu"], F["sshn_u"], F["hv"], F["sshn_v"], F["sshn_t"])

    def bc_open():
        D.psy.invoke_bc_open(prm, ssh_bc, F["ssha"], F["ua"], F["va"], *bc, stream=s)

    def bc_three():
        D.psy.invoke_bc_ssh(F["ssha"], ssh_bc, stream=s)
        D.psy.invoke_bc_flather_u(prm, F["ua"], F["hu"], F["sshn_u"], F["sshn_t"], stream=s)
        D.psy.invoke_bc_flather_v(prm, F["va"], F["hv"], F["sshn_v"], F["sshn_t"], stream=s)

    def momentum():
        D.psy.invoke_momentum(prm, F["ua"], F["va"], *mom, stream=s)

    def step():
        D.psy.invoke_continuity(F["ssha"], F["sshn_t"], F["sshn_u"], F["sshn_v"], F["hu"], F["hv"], F["un"], F["vn"], 20.0,
                                stream=s)
        D.psy.invoke_next_sshu(F["ssha_u"], F["ssha"], stream=s)
        D.psy.invoke_next_sshv(F["ssha_v"], F["ssha"], stream=s)
        momentum()
        bc_open()

    variants = {"bc_open": bc_open, "bc_three_launches": bc_three, "momentum_fused": momentum, "step": step}
    launches = {1024: 200, 4096: 40, 8192: 10}[n]
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
    med = {k: statistics.median(v) for k, v in times.items()}
    r = {"open_T": plan.nt, "open_u": plan.nu, "open_v": plan.nv, "launches_per_window": launches, "ms": med,
         "ms_all_windows": times, "bc_open_over_momentum": med["bc_open"] / med["momentum_fused"],
         "bc_open_share_of_step": med["bc_open"] / med["step"],
         "three_launches_over_momentum": med["bc_three_launches"] / med["momentum_fused"],
         "three_launches_share_of_step_with_them": med["bc_three_launches"] / (med["step"] - med["bc_open"] +
                                                                                med["bc_three_launches"])}
    result["sizes"][str(n)] = r
    print(n, json.dumps({k: round(v, 5) for k, v in med.items()}), "bc_open share %.4f, three launches share %.4f"
          % (r["bc_open_share_of_step"], r["three_launches_share_of_step_with_them"]), flush=True)
    del F, mom, bc, g, plan
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
print("wrote", out_path)
