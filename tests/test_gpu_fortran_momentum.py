"""GPU test (-m gpu): the Fortran wrappers of the momentum and next_ssh kernels through a small program
(tests/fortran/ftest_momentum.f90, built by the Fortran layer's Makefile like every program there).  On a grid with a -1/0/1
user tmask the program runs invoke_next_sshu / invoke_next_sshv, invoke_momentum_u + invoke_momentum_v and invoke_momentum after
momentum_coriolis, and writes the grid, its host-computed fcor_u / fcor_v, the inputs and the outputs to a file; every output
must equal tests/momentum_numpy.py on those inputs bit for bit (an argument out of order in a bind(C) interface or a wrapper
shows up as a differing array).  Without momentum_coriolis a momentum wrapper must stop."""
import math
import os
import subprocess

import numpy as np
import pytest

import momentum_numpy as M
from conftest import ROOT

pytestmark = pytest.mark.gpu
FDIR = os.path.join(ROOT, "dl_esm_inf_amd", "fortran")
EXE = os.path.join(FDIR, "build", "ftest_momentum.exe")
PRM = M.params(20.0, 0.00015, 50.0, 9.80665)


def _run(*args, alignment=None):
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DL_ESM_ALIGNMENT"):
        env.pop(k, None)
    if alignment:
        env["DL_ESM_ALIGNMENT"] = str(alignment)
    return subprocess.run([EXE, *map(str, args)], env=env, capture_output=True, text=True, timeout=300)


def _read(path):
    """the program's file: extents, U / V internal regions, tmask, 11 grid arrays, 10 inputs, 6 outputs"""
    raw = open(path, "rb").read()
    head = np.frombuffer(raw, dtype=np.int32, count=10)
    nx, ny = int(head[0]), int(head[1])
    ub, vb = tuple(int(x) for x in head[2:6]), tuple(int(x) for x in head[6:10])
    off = 40
    tm = np.frombuffer(raw, dtype=np.int32, count=nx * ny, offset=off).reshape(ny, nx)
    off += 4 * nx * ny
    rest = np.frombuffer(raw, dtype=np.float64, offset=off).reshape(-1, ny, nx)
    assert rest.shape[0] == 11 + 10 + 6
    return nx, ny, ub, vb, tm, [a.copy() for a in rest]


@pytest.mark.parametrize("nx,ny,alignment", [(130, 70, 64), (37, 21, None), (4, 3, 8)])
def test_fortran_momentum_wrappers_match_the_checker(tmp_path, nx, ny, alignment):
    out = str(tmp_path / "momentum.bin")
    p = _run(nx, ny, "run", out, alignment=alignment)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert "G: wrote" in p.stdout
    gnx, gny, ub, vb, tm, arrs = _read(out)
    grid = dict(zip(("dx_t", "dy_t", "dx_u", "dy_u", "dx_v", "dy_v", "area_t", "area_u", "area_v", "fcor_u", "fcor_v"), arrs[:11]))
    G = M.SimpleNamespace(tmask=tm, **grid)
    assert (tm == -1).any() and (tm == 0).any() and (tm == 1).any()
    f50 = (2.0 * 7.292116e-5) * math.sin(50.0 * (math.pi / 180.0))          # grid_init's f-plane, with the host's sin
    assert np.allclose(G.fcor_u, f50, rtol=4e-16, atol=0) and np.allclose(G.fcor_v, f50, rtol=4e-16, atol=0)
    H = arrs[11:21]
    ua, va, ua2, va2, sshu, sshv = arrs[21:]
    want_u, want_v = np.full((gny, gnx), -7.0), np.full((gny, gnx), -7.0)
    M.momentum_u(PRM, G, ub, *H[:9], want_u)
    M.momentum_v(PRM, G, vb, *H[:8], H[9], want_v)
    assert M.same(ua, want_u) and M.same(va, want_v)
    assert M.same(ua2, want_u) and M.same(va2, want_v)
    if nx > 8:
        assert (want_u != -7.0).any() and (want_v != -7.0).any()
    for got, fn, area, box in ((sshu, M.next_sshu, G.area_u, ub), (sshv, M.next_sshv, G.area_v, vb)):
        want = np.full((gny, gnx), -7.0)
        fn(box, G.tmask, G.area_t, area, H[3], want)
        assert M.same(got, want)


def test_fortran_momentum_stops_without_coriolis(tmp_path):
    p = _run(40, 30, "nocor", str(tmp_path / "unused.bin"), alignment=64)
    assert p.returncode != 0, p.stdout[-2000:]
    assert "momentum_coriolis" in (p.stdout + p.stderr).replace("\n ", ""), (p.stdout[-2000:], p.stderr[-2000:])
    assert "G: momentum without coriolis ran" not in p.stdout
