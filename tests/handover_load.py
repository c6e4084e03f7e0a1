"""A COMPETING LOAD for the hand-over tests (tests/test_a_handover_load_gpu.py), in a process of its own so that its hardware
queues are its own: short launches of libdlesm_lab.so's load kernels back to back on one stream of device 0, while the
workers run the distributed steps.  No launch waits for anything: fixed trip counts, one launch 0.08-0.25 ms, so a consumer
that spins on a flag is never kept from its producer for longer than that -- and so that the shortest pass window of the
workers (about a millisecond: 160 mailbox steps of the 8x3 tile) still holds three whole launches.

    python tests/handover_load.py PATTERN      PATTERN = few | lopsided | stream | none

  few       3 workgroups, long: 3 of the 8 XCDs carry one busy CU each
  lopsided  8k + 3 workgroups, one per CU (they claim the LDS), just over the CU count: 3 XCDs always have one more queued
  stream    dlesm_lab_stream_copy_f64 over two arrays of 512 MiB, one half of them per launch in turn: evicts the L2s and
            the Infinity Cache, loads the fabric
  none      nothing is launched (the control)

Three launches are kept in flight; the host waits for the oldest one's event and logs time.monotonic_ns(), so the queue
never runs dry between launches.  Prints `LOAD RUNNING` once the first launch has completed, stops on a line on stdin (or
after 120 s) and prints `LOAD LOG {...}`: the completion time of every launch, the calibrated launch time and trip count, and
busy_fraction = launches x calibrated launch time / elapsed (above 1 where a launch runs faster than when calibrated alone,
below where the workers' kernels share the chip).
overlap_counts() below is the arithmetic the tests apply to that log and to the windows the workers print."""
import bisect
import collections
import json
import os
import select
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERNS = ("few", "lopsided", "stream", "none")
DEPTH = 3                    # launches kept in flight: the queue never runs dry while the host logs a completion, and every
                             # entry of the log is ONE launch, so ">= 3 inside" counts launches
MAX_ITERS = 1 << 16          # hard upper bound of the calibration (the C entry refuses more than 2^20)
SLICE = 4096                 # doubles per workgroup: 32 KiB, read and written `iters` times
LIFETIME_S = 120.0
MIN_INSIDE = 3


def overlap_counts(log, t0, t1):
    """(before, inside, after): how many of the load's completion times (ns, CLOCK_MONOTONIC) lie before the window
    [t0, t1], inside it (ends included) and after it; `log` ascends, as the load writes it"""
    before = bisect.bisect_left(log, t0)
    after = len(log) - max(before, bisect.bisect_right(log, t1))
    return before, len(log) - before - after, after


def window_is_loaded(log, t0, t1, min_inside=MIN_INSIDE):
    """was the load running before, throughout and after the window?  A completion before t0, one after t1 and at least
    `min_inside` inside; an empty or reversed window is never loaded"""
    if t1 <= t0:
        return False
    before, inside, after = overlap_counts(log, t0, t1)
    return before >= 1 and after >= 1 and inside >= min_inside


def _stop_requested():
    r, _, _ = select.select([sys.stdin], [], [], 0)
    return bool(r)


def main():
    pattern = sys.argv[1]
    assert pattern in PATTERNS, pattern
    sys.path.insert(0, ROOT)
    import ctypes as C

    import torch

    import dl_esm_inf_amd as D
    torch.cuda.set_device(0)
    torch.zeros(1, device="cuda")                       # the device is open in every pattern, `none` included
    torch.cuda.synchronize()
    info = {"pattern": pattern, "iters": 0, "launch_ms": 0.0, "groups": 0}
    launch = None
    if pattern != "none":
        lab = D._cabi.lab()
        s = torch.cuda.Stream()
        sp = C.c_void_p(s.cuda_stream)
        if pattern == "stream":
            n = (512 << 20) // 8                         # 512 MiB per array, swept in two launches of 256 + 256 MiB
            with torch.cuda.stream(s):
                a, b = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
            halves = [((C.c_void_p * 1)(a.data_ptr() + h * 4 * n), (C.c_void_p * 1)(b.data_ptr() + h * 4 * n)) for h in (0, 1)]
            turn = [0]

            def launch():
                src, dst = halves[turn[0] & 1]
                turn[0] += 1
                D._cabi.check_lab(lab.dlesm_lab_stream_copy_f64(1, 1, src, dst, n // 2, 0, sp))
        else:
            cus = torch.cuda.get_device_properties(0).multi_processor_count
            groups = 3 if pattern == "few" else 8 * (cus // 8) + 3
            one_per_cu = 0 if pattern == "few" else 1
            with torch.cuda.stream(s):
                buf = torch.ones(groups * SLICE, dtype=torch.float64, device="cuda")
            info["groups"] = groups
            if one_per_cu:                               # the premise of `lopsided`, as the runtime sees it
                occ = C.c_int(0)
                D._cabi.check_lab(lab.dlesm_lab_load_rmw_occupancy(1, C.byref(occ)))
                assert occ.value == 1, f"a CU holds {occ.value} workgroups of the LDS-claiming kernel, not one"
                info["workgroups_per_cu"] = occ.value

            def launch():
                D._cabi.check_lab(lab.dlesm_lab_load_rmw_f64(buf.data_ptr(), buf.numel(), groups, SLICE, info["iters"],
                                                             one_per_cu, sp))

        def timed():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            launch()                                     # (warm: the first launch of a kernel loads its code object)
            e0.record(s)
            launch()
            e1.record(s)
            s.synchronize()
            return e0.elapsed_time(e1)

        if pattern == "stream":
            info["launch_ms"] = timed()
        else:
            # calibrate once: from a small trip count up, at least doubling, until one launch takes 0.08-0.25 ms (aim: 0.1)
            info["iters"] = 8
            while True:
                ms = timed()
                if ms >= 0.08 or info["iters"] >= MAX_ITERS:
                    break
                aim = int(info["iters"] * 0.1 / ms) if ms > 0.03 else 0      # (below 30 us the launch itself is what is timed)
                info["iters"] = min(MAX_ITERS, max(info["iters"] * 2, aim))
            info["launch_ms"] = ms
    log = []
    end = time.monotonic() + LIFETIME_S
    if launch is None:
        print("LOAD RUNNING", flush=True)
        select.select([sys.stdin], [], [], LIFETIME_S)
    else:
        pending = collections.deque()
        while time.monotonic() < end and not _stop_requested():
            launch()
            ev = torch.cuda.Event()
            ev.record(s)
            pending.append(ev)
            if len(pending) >= DEPTH:                    # wait for the OLDEST launch only: DEPTH - 1 stay queued behind it
                pending.popleft().synchronize()
                log.append(time.monotonic_ns())
                if len(log) == 1:
                    print("LOAD RUNNING", flush=True)
        while pending:
            pending.popleft().synchronize()
            log.append(time.monotonic_ns())
        info["busy_fraction"] = info["launch_ms"] * 1e6 * len(log) / max(1, log[-1] - log[0]) if len(log) > 1 else 0.0
    print("LOAD LOG " + json.dumps(dict(info, depth=DEPTH, completions=log)), flush=True)


if __name__ == "__main__":
    main()
