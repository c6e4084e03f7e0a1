"""GPU test (-m gpu): the Jacobi step with its residual on a decomposed grid (psy.invoke_jacobi5_residual, dlesm_global_max_f64)
between PROCESSES -- 2 and 4 ranks sharing the one GPU in mailbox mode (tests/jacobi_residual_worker.py): a Laplace solve of
pipelined distributed steps with the residual every 5 steps, against the oracle's loop on the undivided domain (the global max
bit for bit at every check, the same stopping step, l2 within 1e-12, valid halos after every residual call), and a global max
with a NaN on one rank.  Sorts before the in-process GPU tests: the pytest process must not have touched the GPU when it starts
children."""
import os
import sys

import pytest

from conftest import ROOT
from rank_world import run_world

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nx,ny,ndx,ndy", [(48, 40, 2, 1),      # x-split
                                         (48, 40, 2, 2)])     # 2 x 2
def test_jacobi_residual_between_processes(nx, ny, ndx, ndy):
    import torch
    assert not torch.cuda.is_initialized(), "run this file before any in-process GPU test"
    world = ndx * ndy
    procs, outs = run_world([sys.executable, os.path.join(ROOT, "tests", "jacobi_residual_worker.py"), str(nx), str(ny), str(ndx),
                             str(ndy)], world)
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{out[-3000:]}"
        assert "ERROR" not in out, out[-3000:]
        assert f"rank {r}: tile" in out and "errors 0 (all ranks 0)" in out, out[-3000:]
        assert "stop at step None" not in out, out[-3000:]
