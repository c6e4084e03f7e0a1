"""GPU test (-m gpu): the device-side hand-overs of the distributed steps under UNEVEN LOAD, with
WARM readers, checking EVERY WORD.  A load process (tests/handover_load.py) keeps a few CUs, a lopsided grid or the whole
memory system busy from queues of its own while tests/handover_load_worker.py runs every form for tens to hundreds of steps
back to back and compares bit for bit with the oracle -- in loop-back, and as 2 and 4 processes on the one GPU.

Two conditions decide a test: every worker is right (exit 0, no ERROR line), and the load's log shows a completed launch
before, at least three inside and one after EVERY pass window the workers printed -- a hand-over that was never under load
has not been tested, so a window without that FAILS the test (pattern `none`, the control, is exempt).
Sorts before the in-process GPU tests: the pytest process must not have touched the GPU when it starts children."""
import json
import os
import socket
import subprocess
import sys
import threading
import time

import pytest

from conftest import ROOT
from handover_load import MIN_INSIDE, PATTERNS, overlap_counts, window_is_loaded

pytestmark = pytest.mark.gpu
WORKER = os.path.join(ROOT, "tests", "handover_load_worker.py")
CASES = {"loopback": (1, ["loopback"]),
         "ranks-2-mailbox": (2, ["ranks", "96x64:64,64x96:none", "mailbox"]),
         "ranks-4-connect": (4, ["ranks", "640x512:64", "connect"])}
DEADLINE_S = 300
LOAD_START_S = 120            # for the load process to open the device, allocate and calibrate


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_under_load(pattern, world, argv, deadline_s=DEADLINE_S):
    """start the load, wait for it, run the world of workers, stop the load: (worker outputs, return codes, load log)"""
    load = subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "handover_load.py"), pattern], stdin=subprocess.PIPE,
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    procs = []
    lines, running = [], threading.Event()

    def read_load():                                         # (a thread, so that waiting for the load has a limit too)
        for line in load.stdout:
            lines.append(line)
            if line.startswith("LOAD RUNNING"):
                running.set()
        running.set()                                        # end of file: the wait below must not outlast the process

    reader = threading.Thread(target=read_load, daemon=True)
    reader.start()
    try:
        running.wait(LOAD_START_S)
        assert any(ln.startswith("LOAD RUNNING") for ln in lines), \
            f"the load process did not start within {LOAD_START_S} s:\n" + "".join(lines)[-3000:]
        port = _free_port()
        for r in range(world):
            env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
            procs.append(subprocess.Popen([sys.executable, WORKER] + argv, env=env, stdout=subprocess.PIPE,
                                          stderr=subprocess.STDOUT, text=True))
        end = time.monotonic() + deadline_s                  # one deadline for the whole world
        outs = []
        for p in procs:
            out, _ = p.communicate(timeout=max(1.0, end - time.monotonic()))
            outs.append(out)
        load.stdin.write("stop\n")
        load.stdin.close()
        load.wait(timeout=60)
        reader.join(timeout=60)
        tail = "".join(lines)
    finally:
        for q in procs + [load]:
            if q.poll() is None:
                q.kill()
    assert load.returncode == 0, "the load process failed:\n" + tail[-3000:]
    logs = [ln for ln in tail.splitlines() if ln.startswith("LOAD LOG ")]
    assert len(logs) == 1, tail[-3000:]
    return outs, [p.returncode for p in procs], json.loads(logs[0][len("LOAD LOG "):])


def windows_of(out):
    """[(form, pass, t0, t1)] from a worker's WINDOW lines"""
    res = []
    for ln in out.splitlines():
        if ln.startswith("WINDOW "):
            _, form, which, t0, t1 = ln.split()
            res.append((form, which, int(t0), int(t1)))
    return res


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("pattern", ["none", "few", "lopsided", "stream"])
def test_handovers_under_load(pattern, case):
    import torch
    assert not torch.cuda.is_initialized(), "run this file before any in-process GPU test"
    assert pattern in PATTERNS
    world, argv = CASES[case]
    wall0 = time.monotonic()
    outs, codes, load = run_under_load(pattern, world, argv)
    wall = time.monotonic() - wall0
    # ---- correctness: every worker exits 0, prints zero errors and no ERROR line
    for r, (rc, out) in enumerate(zip(codes, outs)):
        assert rc == 0, f"rank {r} failed:\n{out[-4000:]}"
        assert "ERROR" not in out, out[-4000:]
        assert f"rank {r}: handover worker" in out and "errors 0 (all ranks 0)" in out, out[-3000:]
    # ---- overlap shown: the load ran before, throughout and after every pass window
    log = load["completions"]
    void, nwin, gpu_ns, fewest = [], 0, 0, None
    for r, out in enumerate(outs):
        wins = windows_of(out)
        assert wins, out[-3000:]
        for form, which, t0, t1 in wins:
            nwin += 1
            gpu_ns += t1 - t0
            before, inside, after = overlap_counts(log, t0, t1)
            fewest = inside if fewest is None else min(fewest, inside)
            if pattern != "none" and not window_is_loaded(log, t0, t1):
                void.append(f"rank {r} {form} pass {which}: {(t1 - t0) / 1e6:.2f} ms, load launches before/inside/after "
                            f"{before}/{inside}/{after}")
    print(f"HANDOVER {pattern} {case}: wall {wall:.1f} s, {nwin} windows, {gpu_ns / 1e6:.1f} ms inside them, load launch "
          f"{load['launch_ms']:.3f} ms (iters {load['iters']}), {len(log)} load launches, busy {load.get('busy_fraction', 0.0):.2f}, "
          f"fewest inside one window {fewest}")
    assert not void, (f"VOID: {len(void)} of {nwin} pass windows were not under load (need one launch before, {MIN_INSIDE} "
                      "inside, one after):\n" + "\n".join(void[:40]))
