"""GPU test (-m gpu): psy.flow_output on a decomposed grid between PROCESSES -- 2 and 4 ranks sharing the one GPU in mailbox
mode (tests/flow_output_worker.py): every rank's internal region holds the bits of tests/flow_output_numpy.py on the undivided
domain for all six outputs, stored and added twice, after the mask's and the velocities' halos --
corners included, which the vorticity reads -- came from the neighbours; the halos of the outputs keep their content; a mask
that leaves one rank all land.  Sorts before the in-process GPU tests: the pytest process must not have touched the GPU when
it starts children."""
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


@pytest.mark.parametrize("nx,ny,ndx,ndy", [(48, 40, 2, 1),      # x-split
                                         (48, 40, 2, 2)])     # 2 x 2
def test_flow_output_between_processes(nx, ny, ndx, ndy):
    import torch
    assert not torch.cuda.is_initialized(), "run this file before any in-process GPU test"
    world = ndx * ndy
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "flow_output_worker.py"), str(nx),
                                       str(ny), str(ndx), str(ndy)], env=env, stdout=subprocess.PIPE,
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
        assert f"rank {r}: {ndx}x{ndy} tiles" in out and "errors 0 (all ranks 0)" in out, out[-3000:]
