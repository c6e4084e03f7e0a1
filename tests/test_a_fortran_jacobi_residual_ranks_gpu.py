"""GPU test (-m gpu): the distributed branch of the Fortran wrapper invoke_jacobi5_residual (tests/fortran/ftest_jacobi_residual.f90,
mode "dm") -- 1, 2 and 4 ranks of the program sharing the one GPU in mailbox mode, on an input that is a function of the global
cell index.  Every rank must print the same bits; the max must be the undivided run's bit for bit, the l2 norm within 1e-12 of
it; and every rank's `out` must hold its neighbours' cells in its depth-1 halos after the calls (the wrapper joins a pipelined
step first and exchanges `out` after, as invoke_jacobi5_dm).  Sorts before the in-process GPU tests: the pytest process must not
have touched the GPU when it starts children."""
import os
import re
import struct
import subprocess
import time

import pytest

from conftest import ROOT
from rank_world import run_world

pytestmark = pytest.mark.gpu
FDIR = os.path.join(ROOT, "dl_esm_inf_amd", "fortran")
EXE = os.path.join(FDIR, "build", "ftest_jacobi_residual.exe")
NX, NY = 130, 100


def _run(world):
    env = dict(LOCAL_RANK="0", DLESM_TRANSPORT="mailbox", DLESM_JOB_ID=f"pytest-{os.getpid()}-{time.time_ns()}",
               DLESM_BOARD_TIMEOUT_S="120", DL_ESM_ALIGNMENT="64")
    procs, outs = run_world([EXE, str(NX), str(NY), "dm", "-"], world, env)
    vals = []
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} of {world} failed:\n{out[-3000:]}"
        m = re.search(r"G: rank (\d+) of (\d+) rmax ([0-9A-F]{16}) rl2 ([0-9A-F]{16}) halo cells differ (\d+)", out)
        assert m, out[-3000:]
        assert int(m.group(2)) == world and int(m.group(5)) == 0, out[-3000:]
        vals.append((m.group(3), m.group(4)))
    return vals


def _f64(hexbits):
    return struct.unpack("<d", struct.pack("<Q", int(hexbits, 16)))[0]


def test_fortran_residual_on_decomposed_grids():
    import torch
    assert not torch.cuda.is_initialized(), "run this file before any in-process GPU test"
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)
    (one_max, one_l2), = _run(1)
    assert _f64(one_max) > 1.0
    for world in (2, 4):
        vals = _run(world)
        assert len(set(vals)) == 1, vals                          # every rank the same bits
        rmax, rl2 = vals[0]
        assert rmax == one_max, (world, _f64(rmax), _f64(one_max))
        assert abs(_f64(rl2) - _f64(one_l2)) <= 1e-12 * _f64(one_l2), (world, _f64(rl2), _f64(one_l2))
