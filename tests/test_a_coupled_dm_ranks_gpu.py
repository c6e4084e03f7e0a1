"""GPU test (-m gpu): decomposition invariance of the coupled step on a decomposed grid (dlesm_nemolite_coupled_step_dm) and
of the mask's int halo exchange (dlesm_halo_exchange_i32) between PROCESSES sharing the one GPU in mailbox mode
(tests/coupled_dm_worker.py): a tidal open channel with an island across the tile boundaries; every rank's mask after
exchange_mask_halos against the global mask's window, and its box and halos of all thirteen flow arrays and both tracers
against the CPU loops on the undivided domain after every step.  4 ranks (2 x 2) on a halo_width = 2 grid, three steps with the
Hancock scheme; 2 ranks (2 x 1) on a halo_width = 1 grid, two steps with the upwind scheme.  Each rank runs under a time limit
of its own, and the first rank to fail ends the others.  Sorts before the in-process GPU tests: the pytest process must not
have touched the GPU when it starts children."""
import os
import socket
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor, as_completed

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
LIMIT = 120          # seconds a rank may take (a healthy run takes a few)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("ndx,ndy,steps,scheme,hw", [(2, 2, 3, "hancock", 2), (2, 1, 2, "upwind", 1)])
def test_coupled_step_dm_between_processes(ndx, ndy, steps, scheme, hw):
    import torch
    assert not torch.cuda.is_initialized(), "run this file before any in-process GPU test"
    nx, ny = 130, 100
    world = ndx * ndy
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen(["timeout", "-k", "10", str(LIMIT), sys.executable,
                                       os.path.join(ROOT, "tests", "coupled_dm_worker.py"), str(nx), str(ny), str(ndx),
                                       str(ndy), str(steps), scheme, str(hw)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
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
