"""GPU test (-m gpu): the particle migration between PROCESSES -- 2 ranks (2 x 1) and 4 ranks (2 x 2) sharing the one GPU in
mailbox mode (tests/particle_migrate_worker.py): a gyre with an island across the tile boundaries, 25 steps of
psy.drifter_step(nsub = 1) followed by psy.particle_migrate with a cap that holds particles back; every rank compares its
slots, its payload and its record with the numpy World of all ranks after every step, bit for bit; at the end every id is in
exactly one slot over all ranks, the wrapper raises on the rank that had to drop arrivals, and no IPC retry or timed-out wait
has been counted.

Each rank runs under a time limit of its own, and the first rank to fail ends the others.  Sorts before the in-process GPU
tests: the pytest process must not have touched the GPU when it starts children."""
import os
import sys

import pytest

from conftest import ROOT

import rank_world

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mesh", [(2, 1), (2, 2)], ids=lambda m: "%dx%d" % m)
def test_particles_migrate_between_processes(mesh):
    import torch
    assert not torch.cuda.is_initialized(), "run this file before any in-process GPU test"
    nx, ny, steps = 64, 48, 25
    world = mesh[0] * mesh[1]
    procs, outs = rank_world.run_world([sys.executable, os.path.join(ROOT, "tests", "particle_migrate_worker.py"), str(nx), str(ny),
                                        str(mesh[0]), str(mesh[1]), str(steps)], world)
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} failed:\n{out[-3000:]}"
        assert "ERROR" not in out, out[-3000:]
        assert f"rank {r}: tile" in out and "errors 0 (all ranks 0)" in out, out[-3000:]
