"""GPU test (-m gpu): the Fortran wrapper of the flow step's stability check through a small program
(tests/fortran/ftest_flow_courant.f90, built by the Fortran layer's Makefile like every program there).  On a grid with a
-1/0/1 user tmask, flow_courant from Fortran must print the record the Python wrapper returns on the same hashed inputs -- the
bits of the four doubles and all the integers; an argument out of order in the bind(C) interface or the wrapper shows up
there -- and that record equals tests/flow_courant_numpy.py in every member.  rdt = 70 on the 1000 m grid with 10 m of water
puts cells on both sides of a gravity-wave number of 1 (asserted on the host)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import flow_courant_numpy as FN
from conftest import ROOT

pytestmark = pytest.mark.gpu
FDIR = os.path.join(ROOT, "dl_esm_inf_amd", "fortran")
EXE = os.path.join(FDIR, "build", "ftest_flow_courant.exe")
RDT, G, VISC = 70.0, 9.80665, 100.0
LIMITS = (1.0, 0.015, 0.0125, 10.5)                    # the program's second call


def _run(*args, alignment=None):
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DL_ESM_ALIGNMENT"):
        env.pop(k, None)
    if alignment:
        env["DL_ESM_ALIGNMENT"] = str(alignment)
    return subprocess.run(["timeout", "-k", "10", "120", EXE, *map(str, args)], env=env, capture_output=True, text=True)


def _bits(x):
    return "%016X" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def _line(what, rec):
    return "G: %s record %s %s 0 0" % (what, " ".join(_bits(x) for x in rec[:4]), " ".join(str(int(x)) for x in rec[4:14]))


@pytest.mark.parametrize("nx,ny,alignment", [(257, 6, 2), (128, 4, 1)])
def test_fortran_wrapper_prints_the_python_wrappers_record(nx, ny, alignment):
    """array shapes (260, 9) -- the tile, three waves a row -- and (131, 7) -- an odd pitch, the general path"""
    p = _run(nx, ny, "70.0", "100.0", alignment=alignment)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    lines = [l.strip() for l in p.stdout.splitlines() if l.startswith("G:")]
    print("\n".join(lines))

    import torch
    import dl_esm_inf_amd as D
    torch.cuda.set_device(0)
    D.parallel_init(0, 1)
    os.environ["DL_ESM_ALIGNMENT"] = str(alignment)
    try:
        g = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
        g.decompose(nx, ny)
        it = g.subdomain.internal
        jj, ii = np.mgrid[1:it.ystop + 2, 1:it.xstop + 2]
        user = ((7 * ii + 13 * jj + (ii * jj) // 5) % 3 - 1).astype(np.int32)
        user[:3, :3] = 0
        D.grid_init(g, 1000.0, 1000.0, tmask=user)
    finally:
        os.environ.pop("DL_ESM_ALIGNMENT", None)
    assert f"G: extents {g.nx} {g.ny}" in lines, lines
    assert (g.nx, g.ny) == (nx + 3, ny + 3)
    T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
    F, H = [], []
    for k, pt in ((2, U), (3, V), (4, T), (7, T)):                           # un vn ht sshn_t
        f = D.r2d_field(g, pt)
        D.psy.hash_init(f, 500 + k)
        d = f.get_data()
        d = 0.4 * d - 0.2 if k in (2, 3) else 10.0 + d if k == 4 else 0.05 * d
        f.set_data(d)
        F.append(f)
        H.append(np.ascontiguousarray(d))
    tm = g.tmask_device.cpu().numpy()
    dx_t, dy_t = g.dx_t_device.cpu().numpy(), g.dy_t_device.cpu().numpy()
    box = F[3].internal.box()
    for what, limits in (("default", FN.LIMITS), ("limits", LIMITS)):
        want = FN.flow_courant(RDT, G, VISC, box, tm, dx_t, dy_t, *H, *limits)
        r = D.psy.flow_courant(RDT, *F, g=G, visc=VISC, gravity_limit=limits[0], advective_limit=limits[1],
                               viscous_limit=limits[2], depth_limit=limits[3])
        got = (*r[:4], *[(at[2] - 1) * g.nx + at[1] - 1 for at in r[4:8]], *r[8:14])
        assert FN.same_record(got, want), (got, want)
        assert _line(what, got) in lines, (_line(what, got), lines)
        assert 0 < want.gravity_over < want.wet and want.invalid == 0
    assert 0 < want.advective_over < want.wet and 0 < want.shallow < want.wet and want.viscous_over == want.wet
    assert "G: ranks 1 1 1 1" in lines
    assert all(at[0] == 1 for at in r[4:8])
