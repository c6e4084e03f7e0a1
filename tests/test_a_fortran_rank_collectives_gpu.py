"""GPU test (-m gpu, because the mailbox transport opens the device): rank_collectives_mod of the Fortran layer between PROCESSES
(tests/fortran/ftest_rank_collectives.f90) -- 1, 2 and 4 ranks sharing the one GPU in mailbox mode.  The program runs no
kernel: it passes functions of get_rank() to place, rank_total, rank_sum and rank_max.  Every rank must print the same lines,
and they must be the closed forms below: the ownership rule of DESIGN.md section 6.14 (the lowest rank that has a cell AND the
global top), the same cases tests/test_rank_collectives.py drives through the Python layer.  Sorts before the in-process GPU
tests: the pytest process must not have touched the GPU when it starts children."""
import os
import struct
import subprocess
import time

import pytest

from conftest import ROOT
from rank_world import run_world

pytestmark = pytest.mark.gpu
FDIR = os.path.join(ROOT, "dl_esm_inf_amd", "fortran")
EXE = os.path.join(FDIR, "build", "ftest_rank_collectives.exe")


def _hex(x):
    return "%016X" % struct.unpack("<Q", struct.pack("<d", x))[0]


def _want(n):
    """the lines of a world of n ranks; rank r = 1 .. n passes the cell 100 + r"""
    cases = [("tie", 2.5, 1, 101),                                   # all tie, all hold: the lowest rank
             ("distinct", 0.25 * n, n, 7 * n),                       # tops 0.25 r, cells 7 r: the last rank
             ("tie-1-empty", 2.5) + ((2, 102) if n > 1 else (0, -1)),     # rank 1 has the top but no cell
             ("nobody", 0.0, 0, -1),
             ("negated", -11.0, 1, 101),                             # minima 10 + r as maxima of -(10 + r): rank 1
             ("lower-top",) + ((3.0, 2, 102) if n > 1 else (1.0, 1, 101))]   # rank 1 has a cell and 1.0, the others 3.0
    lines = [f"C: {name} top {_hex(top)} owner {owner} index {index}" for name, top, owner, index in cases]
    return lines + [f"C: total small {n * (n + 1) // 2}", f"C: total large {n * 2**40 + n * (n + 1) // 2}",
                    f"C: sum {_hex(0.25 * n * (n + 1))}", f"C: max {_hex(-1.5)}"]


@pytest.mark.parametrize("world", [1, 2, 4])
def test_fortran_place_and_totals_between_processes(world):
    import torch
    assert not torch.cuda.is_initialized(), "run this file before any in-process GPU test"
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)
    env = dict(LOCAL_RANK="0", DLESM_TRANSPORT="mailbox", DLESM_JOB_ID=f"pytest-{os.getpid()}-{time.time_ns()}",
               DLESM_BOARD_TIMEOUT_S="120", DL_ESM_ALIGNMENT="64")
    procs, outs = run_world([EXE], world, env)
    want = _want(world)
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, f"rank {r} of {world} failed:\n{out[-3000:]}"
        got = [line.strip() for line in out.splitlines() if line.lstrip().startswith("C: ")]
        assert got == want, (r, world, out[-3000:])
