"""GPU test (-m gpu): the Fortran wrapper of the Jacobi step with its residual (invoke_jacobi5_residual of dlesm_psy_mod, DESIGN.md
section 5.4) through a small program (tests/fortran/ftest_jacobi_residual.f90).  On one rank, for both norms, it must return the
same bits as psy.invoke_jacobi5_residual on the same data, and write the same `out`; the max must be numpy's.  An unknown norm
must stop the program."""
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
FDIR = os.path.join(ROOT, "dl_esm_inf_amd", "fortran")
EXE = os.path.join(FDIR, "build", "ftest_jacobi_residual.exe")


def _run(*args, alignment=None):
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DL_ESM_ALIGNMENT"):
        env.pop(k, None)
    if alignment:
        env["DL_ESM_ALIGNMENT"] = str(alignment)
    return subprocess.run([EXE, *map(str, args)], env=env, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("nx,ny,alignment", [(300, 90, 64), (37, 21, None)])
def test_fortran_residual_equals_the_python_wrapper(tmp_path, monkeypatch, nx, ny, alignment):
    out = str(tmp_path / "resid.bin")
    p = _run(nx, ny, "run", out, alignment=alignment)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert "G: residuals written" in p.stdout, p.stdout[-2000:]
    raw = open(out, "rb").read()
    ld, nyy = np.frombuffer(raw, np.int32, 2)
    box = tuple(int(v) for v in np.frombuffer(raw, np.int32, 4, 8))
    arrs = np.frombuffer(raw, np.float64, 3 * ld * nyy, 24).reshape(3, nyy, ld)
    fr_max, fr_l2 = np.frombuffer(raw, np.float64, 2, 24 + 8 * 3 * ld * nyy)

    import torch
    import dl_esm_inf_amd as D
    torch.cuda.set_device(0)
    D.parallel_init(0, 1)
    if alignment:
        monkeypatch.setenv("DL_ESM_ALIGNMENT", str(alignment))
    else:
        monkeypatch.delenv("DL_ESM_ALIGNMENT", raising=False)
    g = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
    g.decompose(nx, ny)
    D.grid_init(g, 1.0, 1.0)
    assert (g.nx, g.ny) == (ld, nyy)
    fin, fmax, fl2 = (D.r2d_field(g, D.GO_T_POINTS) for _ in range(3))
    assert fmax.internal.box() == box
    fin.set_data(arrs[0])
    fmax.set_data(np.zeros((nyy, ld)))
    fl2.set_data(np.zeros((nyy, ld)))
    py_max = D.psy.invoke_jacobi5_residual(fmax, fin, "max")
    py_l2 = D.psy.invoke_jacobi5_residual(fl2, fin, "l2")
    assert np.array_equal(fmax.get_data(), arrs[1]) and np.array_equal(fl2.get_data(), arrs[2])
    assert np.float64(py_max).tobytes() == fr_max.tobytes(), (py_max, fr_max)
    assert np.float64(py_l2).tobytes() == fr_l2.tobytes(), (py_l2, fr_l2)
    xs, xe, ys, ye = box
    d = (arrs[1] - arrs[0])[ys - 1:ye, xs - 1:xe]
    assert fr_max == np.max(np.abs(d)) and fr_max > 1.0
    want = math.sqrt(math.fsum((d * d).ravel()))
    assert abs(fr_l2 - want) <= 1e-12 * want


def test_fortran_residual_stops_on_an_unknown_norm(tmp_path):
    p = _run(40, 30, "badnorm", str(tmp_path / "x.bin"), alignment=64)
    assert p.returncode != 0, p.stdout[-2000:]
    assert "is not 'max' or 'l2'" in (p.stdout + p.stderr).replace("\n ", ""), (p.stdout[-2000:], p.stderr[-2000:])
    assert "G: an unknown norm returned" not in p.stdout
