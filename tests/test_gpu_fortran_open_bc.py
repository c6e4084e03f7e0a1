"""GPU test (-m gpu): the Fortran wrappers of the open-boundary kernels through a small program
(tests/fortran/ftest_open_bc.f90, built by the Fortran layer's Makefile like every program there).  On a channel mask -- open
west and east columns and an open south row -- the program runs invoke_bc_ssh, invoke_bc_flather_u and invoke_bc_flather_v, and
invoke_bc_open on a second set of outputs, and writes the grid, the inputs and the outputs to a file; every output must equal
tests/open_bc_numpy.py on those inputs bit for bit (an argument out of order in a bind(C) interface or a wrapper shows up as a
differing array).  On a mask the plan refuses, a wrapper must stop."""
import math
import os
import subprocess

import numpy as np
import pytest

import open_bc_numpy as B
from conftest import ROOT

pytestmark = pytest.mark.gpu
FDIR = os.path.join(ROOT, "dl_esm_inf_amd", "fortran")
EXE = os.path.join(FDIR, "build", "ftest_open_bc.exe")
PRM = B.params(20.0, 0.00015, 50.0, 9.80665)


def _run(*args, alignment=None):
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DL_ESM_ALIGNMENT"):
        env.pop(k, None)
    if alignment:
        env["DL_ESM_ALIGNMENT"] = str(alignment)
    return subprocess.run([EXE, *map(str, args)], env=env, capture_output=True, text=True, timeout=300)


def _read(path):
    """the program's file: extents, T / U / V internal regions, tmask, ssh_bc, 5 inputs, 6 outputs"""
    raw = open(path, "rb").read()
    head = np.frombuffer(raw, dtype=np.int32, count=14)
    nx, ny = int(head[0]), int(head[1])
    boxes = [tuple(int(x) for x in head[2 + 4 * k:6 + 4 * k]) for k in range(3)]
    off = 56
    tm = np.frombuffer(raw, dtype=np.int32, count=nx * ny, offset=off).reshape(ny, nx)
    off += 4 * nx * ny
    ssh_bc = float(np.frombuffer(raw, dtype=np.float64, count=1, offset=off)[0])
    rest = np.frombuffer(raw, dtype=np.float64, offset=off + 8).reshape(-1, ny, nx)
    assert rest.shape[0] == 5 + 6
    return nx, ny, boxes, tm, ssh_bc, [a.copy() for a in rest]


@pytest.mark.parametrize("nx,ny,alignment", [(130, 70, 64), (37, 21, None)])
def test_fortran_open_bc_wrappers_match_the_checker(tmp_path, nx, ny, alignment):
    out = str(tmp_path / "open_bc.bin")
    p = _run(nx, ny, "run", out, alignment=alignment)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert "G: wrote" in p.stdout
    gnx, gny, (tb, ub, vb), tm, ssh_bc, arrs = _read(out)
    assert ssh_bc == B.tide(0.1, 2.0 * math.pi / 43200.0, 1500.0) and ssh_bc != 0.0
    hu, sshn_u, hv, sshn_v, sshn_t = arrs[:5]
    outs = arrs[5:]
    want = [np.full((gny, gnx), -7.0)]
    for k in (1, 2):                                   # the program's initial ua / va
        i, j = np.meshgrid(np.arange(1, gnx + 1), np.arange(1, gny + 1))
        want.append(0.001 * ((13 * i + 7 * j) % 101 - 50).astype(np.float64))
    assert B.refusal(tm, ub, vb) is None
    B.bc_open(PRM, tb, ub, vb, tm, ssh_bc, hu, sshn_u, hv, sshn_v, sshn_t, *want)
    for k in range(3):
        assert B.same(outs[k], want[k]), k
        assert B.same(outs[3 + k], want[k]), k
    assert (want[0] == ssh_bc).sum() == 2 * (ny - 1) + (nx - 2)
    init_u = 0.001 * ((13 * np.arange(1, gnx + 1)[None, :] + 7 * np.arange(1, gny + 1)[:, None]) % 101 - 50)
    assert (want[1] != init_u).sum() == 2 * (ny - 2)   # the open west and east faces of every row between the open row and the land
    assert (want[2] != init_u).sum() == nx - 2         # the open south faces


def test_fortran_open_bc_stops_on_a_refused_mask(tmp_path):
    p = _run(40, 30, "refuse", str(tmp_path / "unused.bin"), alignment=64)
    assert p.returncode != 0, p.stdout[-2000:]
    assert "open inner face" in (p.stdout + p.stderr).replace("\n ", ""), (p.stdout[-2000:], p.stderr[-2000:])
    assert "G: refused mask ran" not in p.stdout
