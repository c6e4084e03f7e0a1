"""GPU test (-m gpu): the Fortran wrappers invoke_shallow_step_x2_dm / invoke_shallow_step_smooth_x2_dm, through a small
program (tests/fortran/ftest_x2_dm.f90, built by the Fortran layer's Makefile like every program there).  On a one-rank
grid decomposed with halo_width = 2 the wrappers hand the C entries a plan without messages, and each distributed entry must
equal its single-domain counterpart bit for bit in all twelve fields (arguments out of order in a bind(C) interface or a
wrapper's call show up as differing fields); on a halo_width = 1 grid the wrapper must stop (gocean_stop)."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
FDIR = os.path.join(ROOT, "dl_esm_inf_amd", "fortran")
EXE = os.path.join(FDIR, "build", "ftest_x2_dm.exe")


def _run(*args, alignment=None):
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DL_ESM_ALIGNMENT"):
        env.pop(k, None)
    if alignment:
        env["DL_ESM_ALIGNMENT"] = str(alignment)
    return subprocess.run([EXE, *map(str, args)], env=env, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("nx,ny,alignment", [(130, 70, 64), (37, 21, None), (4, 3, 8)])
def test_fortran_x2_dm_equals_single_domain(nx, ny, alignment):
    p = _run(nx, ny, "same", alignment=alignment)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert "G: x2 0" in p.stdout and "G: smooth_x2 0" in p.stdout, p.stdout[-2000:]


def test_fortran_x2_dm_refuses_halo_width_1():
    p = _run(40, 30, "hw1", alignment=64)
    assert p.returncode != 0, p.stdout[-2000:]
    assert "halo_width = 2" in (p.stdout + p.stderr).replace("\n ", ""), (p.stdout[-2000:], p.stderr[-2000:])
    assert "G: x2" not in p.stdout
