"""GPU test (-m gpu): decomposition invariance of the one-call NEMOLite2D-class step on a decomposed grid
(dlesm_nemolite_step_dm) between PROCESSES -- 2, 4 and 6 ranks sharing the one GPU in mailbox mode
(tests/nemolite_step_dm_worker.py): a closed basin and a tidal open channel, 20 steps each, every rank's box and depth-1 halos
against the CPU restatements on the undivided domain after every step.  Sorts before the in-process GPU tests: the pytest
process must not have touched the GPU when it starts children."""
import os
import socket
import subprocess
import sys
import time

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("nx,ny,ndx,ndy,steps", [(130, 100, 2, 1, 20),     # x-split
                                                 (130, 100, 1, 2, 20),     # y-split
                                                 (130, 100, 2, 2, 20),     # 2 x 2: every tile has two sides without a neighbour
                                                 (300, 200, 2, 3, 20)])    # 2 x 3: middle tiles have three neighbour sides
def test_nemolite_step_dm_between_processes(nx, ny, ndx, ndy, steps):
    import torch
    assert not torch.cuda.is_initialized(), "run this file before any in-process GPU test"
    world = ndx * ndy
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "nemolite_step_dm_worker.py"), str(nx),
                                       str(ny), str(ndx), str(ndy), str(steps)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs = []
    deadline = time.monotonic() + 300                # ONE deadline for the whole world
    for p in procs:
        try:
            out, _ = p.communicate(timeout=max(1.0, deadline - time.monotonic()))
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            for q in procs:
                q.wait()
            raise
        outs.append(out)
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{out[-3000:]}"
        assert "ERROR" not in out, out[-3000:]
        assert f"rank {r}: tile" in out and "errors 0 (all ranks 0)" in out, out[-3000:]
