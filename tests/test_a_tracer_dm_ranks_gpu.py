"""GPU test (-m gpu): decomposition invariance of tracer transport on a decomposed grid between PROCESSES -- 4 ranks (2 x 2)
sharing the one GPU in mailbox mode, one case per scheme, one after the other:

    upwind   dlesm_tracer_step_dm (tests/tracer_dm_worker.py): a tidal open channel with an island across the tile boundaries,
             three steps of invoke_nemolite_step_dm + invoke_tracer_step_dm with two tracers, every rank's box and depth-1
             halos, of the flow arrays and of the tracers, against the CPU loop on the undivided domain after every step.
    muscl    dlesm_tracer_step_muscl_dm (tests/tracer_limited_dm_worker.py muscl): an open channel's mask with an island
             across the tile boundaries, a fixed random flow, three steps of invoke_tracer_step_muscl_dm with two tracers,
             every rank's box and depth-2 halos against the CPU restatement on the undivided domain after every step.
    hancock  dlesm_tracer_step_hancock_dm (tests/tracer_limited_dm_worker.py hancock): as muscl, through
             invoke_tracer_step_hancock_dm at an rdt that runs both branches of the time-centred factor.

Each rank runs under a time limit of its own, and the first rank to fail ends the others.  Sorts before the in-process GPU
tests: the pytest process must not have touched the GPU when it starts children."""
import os
import socket
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor, as_completed

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
LIMIT = 120          # seconds a rank may take (a healthy run takes a few)
WORKERS = {"upwind": ["tracer_dm_worker.py"], "muscl": ["tracer_limited_dm_worker.py", "muscl"],
           "hancock": ["tracer_limited_dm_worker.py", "hancock"]}


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("scheme", list(WORKERS))
def test_tracer_step_dm_between_processes(scheme):
    import torch
    assert not torch.cuda.is_initialized(), "run this file before any in-process GPU test"
    nx, ny, ndx, ndy, steps = 130, 100, 2, 2, 3
    world = ndx * ndy
    port = _free_port()
    worker, *args = WORKERS[scheme]
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen(["timeout", "-k", "10", str(LIMIT), sys.executable, os.path.join(ROOT, "tests", worker),
                                       *args, str(nx), str(ny), str(ndx), str(ndy), str(steps)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    # the first rank that fails ends the run: nothing goes on using the GPU behind a failure
    outs, failed = [None] * world, None
    with ThreadPoolExecutor(max_workers=world) as pool:
        waits = {pool.submit(p.communicate): r for r, p in enumerate(procs)}
        for done in as_completed(waits):
            r = waits[done]
            outs[r] = done.result()[0]
            if procs[r].returncode != 0 and failed is None:
                failed = r
                for q in procs:
                    if q.poll() is None:
                        q.terminate()
    assert failed is None, f"rank {failed} failed first (exit {procs[failed].returncode}):\n{outs[failed][-3000:]}"
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{out[-3000:]}"
        assert "ERROR" not in out, out[-3000:]
        assert f"rank {r}: tile" in out and "errors 0 (all ranks 0)" in out, out[-3000:]
