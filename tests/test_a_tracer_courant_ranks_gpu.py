"""GPU test (-m gpu): psy.tracer_courant and psy.tracer_courant_check on a decomposed grid between PROCESSES -- 2 and 4 ranks
sharing the one GPU in mailbox mode (tests/tracer_courant_worker.py): every rank gets the record of the undivided domain from
tests/tracer_courant_numpy.py and the lowest rank that owns a cell with each maximum, at an rdt below
both limits and at one beyond them, where tracer_courant_check raises on all ranks; a mask that leaves one rank without a wet
cell still gives the global record there; a NaN depth on one rank is an invalid cell on all.  Sorts before the in-process GPU
tests: the pytest process must not have touched the GPU when it starts children."""
import os
import sys

import pytest

from conftest import ROOT
from rank_world import run_world

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("nx,ny,ndx,ndy", [(48, 40, 2, 1),      # x-split
                                         (48, 40, 2, 2)])     # 2 x 2
def test_tracer_courant_between_processes(nx, ny, ndx, ndy):
    import torch
    assert not torch.cuda.is_initialized(), "run this file before any in-process GPU test"
    world = ndx * ndy
    procs, outs = run_world([sys.executable, os.path.join(ROOT, "tests", "tracer_courant_worker.py"), str(nx), str(ny), str(ndx),
                             str(ndy)], world)
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{out[-3000:]}"
        assert "ERROR" not in out, out[-3000:]
        assert f"rank {r}: {ndx}x{ndy} tiles" in out and "errors 0 (all ranks 0)" in out, out[-3000:]
