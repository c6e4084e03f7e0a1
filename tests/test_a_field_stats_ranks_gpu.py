"""GPU test (-m gpu): field_stats and psy.run_health on a decomposed grid between PROCESSES -- 2 and 4 ranks sharing the one GPU
in mailbox mode (tests/field_stats_worker.py): every rank gets the numbers of the undivided field (min, max, count and
nonfinite exactly, the sums within the worst-case bound of any summation order), a NaN on one rank shows on all, run_health
raises on all ranks and names the owning rank, and a mask that leaves one rank without a wet cell still gives the global
numbers there.  Sorts before the in-process GPU tests: the pytest process must not have touched the GPU when it starts
children."""
import os
import sys

import pytest

from conftest import ROOT
from rank_world import run_world

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nx,ny,ndx,ndy", [(48, 40, 2, 1),      # x-split
                                         (48, 40, 2, 2)])     # 2 x 2
def test_field_stats_between_processes(nx, ny, ndx, ndy):
    import torch
    assert not torch.cuda.is_initialized(), "run this file before any in-process GPU test"
    world = ndx * ndy
    procs, outs = run_world([sys.executable, os.path.join(ROOT, "tests", "field_stats_worker.py"), str(nx), str(ny), str(ndx),
                             str(ndy)], world)
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{out[-3000:]}"
        assert "ERROR" not in out, out[-3000:]
        assert f"rank {r}: tile" in out and "errors 0 (all ranks 0)" in out, out[-3000:]
