"""GPU test (-m gpu): the Fortran cell-bin wrapper through a small program
(tests/fortran/ftest_cell_bin.f90, built by the Fortran layer's Makefile like every program there).  On the grid and the
particles of the particle-sort program, cell_bin into a T-point field filled with -3 must give the restatement's counts
(tests/cell_bin_numpy.py) over the T internal region -- the program prints their sum and a hash -- and leave everything
outside at -3; two additions with alpha = 0.5 must be two roundings each and touch no empty cell, and a particle_sort must
not change the count, which the program checks itself; an argument out of order in the bind(C) interface or the wrapper
shows up there."""
import os
import subprocess

import numpy as np
import pytest

import cell_bin_numpy as BN
import particle_order_numpy as PN
from conftest import ROOT

pytestmark = pytest.mark.gpu
FDIR = os.path.join(ROOT, "dl_esm_inf_amd", "fortran")
EXE = os.path.join(FDIR, "build", "ftest_cell_bin.exe")
MASK64 = (1 << 64) - 1
BOX = (2, 24, 2, 20)          # the T internal region of the 26 x 22 grid (the program prints it)


def _run(*args, alignment=None):
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DL_ESM_ALIGNMENT"):
        env.pop(k, None)
    if alignment:
        env["DL_ESM_ALIGNMENT"] = str(alignment)
    return subprocess.run(["timeout", "-k", "10", "120", EXE, *map(str, args)], env=env, capture_output=True, text=True)


def _hash(a):
    """the program's hash: h = rotl(h, 5) ^ value over the elements in order"""
    h = 0
    for b in a.astype(np.int64).view(np.uint64).tolist():
        h = (((h << 5) | (h >> 59)) & MASK64) ^ b
    return "%016X" % h


@pytest.mark.parametrize("n,alignment", [(1000, 2), (65, 1)])
def test_the_count_is_the_restatements(n, alignment):
    p = _run(n, alignment=alignment)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    lines = [l.strip() for l in p.stdout.splitlines() if l.startswith("G:")]
    print("\n".join(lines))
    p1 = np.arange(n)
    px = 0.5 + 0.125 * ((37 * p1) % 211)
    py = 0.5 + 0.0625 * ((101 * p1) % 353)
    st = np.where((p1 + 1) % 11 == 0, 1 + (p1 + 1) % 3, 0).astype(np.int32)
    perm, nlive = PN.order(BOX, px, py, st)
    S, has, unordered = BN.sums_array(BOX, px, py, st, perm, [None])
    assert unordered == 0 and S[0].sum() == nlive and n // 4 < nlive < n - n // 11 and not has.all()
    assert "G: extents 26 22 region %d %d %d %d" % BOX in lines, lines
    assert "G: count sum %d hash %s outside T" % (nlive, _hash(S[0])) in lines, lines
    assert "G: added twice T" in lines, lines
    assert "G: the same after a sort T" in lines, lines
