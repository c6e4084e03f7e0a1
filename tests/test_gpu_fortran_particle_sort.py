"""GPU test (-m gpu): the Fortran particle-order wrappers through a small program
(tests/fortran/ftest_particle_sort.f90, built by the Fortran layer's Makefile like every program there).  On the grid, the flow
and the particles of the drifter program, particle_sort then drifter_step then drifters_get and particle_origin must reproduce
the unsorted run through origin, bit for bit, which the program checks itself; the origin it prints (1-based) must be the
restatement's permutation (tests/particle_order_numpy.py) over the T internal region, nlive its count of live particles, and
origin must be the identity and nlive -1 before the first sort; an argument out of order in the bind(C) interfaces or the
wrappers shows up there."""
import os
import subprocess

import numpy as np
import pytest

import particle_order_numpy as PN
from conftest import ROOT

pytestmark = pytest.mark.gpu
FDIR = os.path.join(ROOT, "dl_esm_inf_amd", "fortran")
EXE = os.path.join(FDIR, "build", "ftest_particle_sort.exe")
MASK64 = (1 << 64) - 1
BOX = (2, 24, 2, 20)          # the T internal region of the 26 x 22 grid (tests/test_gpu_fortran_drifter.py asserts it)


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
def test_the_sorted_run_reproduces_the_unsorted_run(n, alignment):
    p = _run(n, alignment=alignment)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    lines = [l.strip() for l in p.stdout.splitlines() if l.startswith("G:")]
    print("\n".join(lines))
    p1 = np.arange(n)
    px = 0.5 + 0.125 * ((37 * p1) % 211)
    py = 0.5 + 0.0625 * ((101 * p1) % 353)
    st = np.where((p1 + 1) % 11 == 0, 1 + (p1 + 1) % 3, 0).astype(np.int32)
    perm, nlive = PN.order(BOX, px, py, st)
    assert n // 4 < nlive < n - n // 11 and (perm != p1).sum() > n // 2
    assert "G: extents 26 22" in lines, lines
    assert "G: before nlive -1 identity T" in lines, lines
    assert "G: sorted nlive %d origin %s moved %d" % (nlive, _hash(perm + 1), int((perm != p1).sum())) in lines, lines
    assert "G: the sorted set holds the particles it was given T" in lines, lines
    assert "G: the sorted run reproduces the unsorted run T stepped T" in lines, lines
    again = [l for l in lines if l.startswith("G: after a second sort T nlive ")]
    assert len(again) == 1 and 0 < int(again[0].split()[-1]) <= nlive, lines
