"""GPU test (-m gpu): the Fortran wrapper of the tracer schemes' Courant check through a small program
(tests/fortran/ftest_tracer_courant.f90, built by the Fortran layer's Makefile like every program there).  On a grid with a
-1/0/1 user tmask, tracer_courant from Fortran must print the record the Python wrapper returns on the same hashed inputs --
the bits of both maxima and all six integers; an argument out of order in the bind(C) interface or the wrapper shows up there
-- and that record equals tests/tracer_courant_numpy.py in every member.  rdt = 1.0e7 on the 1000 m grid puts faces on both
sides of a Courant number of 1 (asserted on the host)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import tracer_courant_numpy as CN
import tracer_hancock_numpy as TH
from conftest import ROOT

pytestmark = pytest.mark.gpu
FDIR = os.path.join(ROOT, "dl_esm_inf_amd", "fortran")
EXE = os.path.join(FDIR, "build", "ftest_tracer_courant.exe")
RDT = 1.0e7


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
    return "G: %s record %s %s %s" % (what, _bits(rec[0]), _bits(rec[1]), " ".join(str(int(x)) for x in rec[2:8]))


@pytest.mark.parametrize("nx,ny,alignment", [(257, 6, 2), (128, 4, 1)])
def test_fortran_wrapper_prints_the_python_wrappers_record(nx, ny, alignment):
    """array shapes (260, 9) -- the tile, three waves a row -- and (131, 7) -- an odd pitch, the general path"""
    p = _run(nx, ny, "1.0e7", alignment=alignment)
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
    for k, pt in enumerate((U, V, T, U, V, T, U, V), start=2):               # un vn ht hu hv sshn_t sshn_u sshn_v
        f = D.r2d_field(g, pt)
        D.psy.hash_init(f, 500 + k)
        d = f.get_data()
        d = 0.4 * d - 0.2 if k in (2, 3) else 10.0 + d if k in (4, 5, 6) else 0.05 * d
        f.set_data(d)
        F.append(f)
        H.append(np.ascontiguousarray(d))
    un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v = H
    tm, area_t = g.tmask_device.cpu().numpy(), g.area_t_device.cpu().numpy()
    box = F[5].internal.box()
    mid, big = TH.face_shares(RDT, box, tm, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v)
    assert mid >= 0.10 and big >= 0.10, (mid, big)
    for what, limits in (("default", (0.5, 1.0)), ("limits 1 2", (1.0, 2.0))):
        want = CN.tracer_courant(RDT, box, tm, area_t, un, vn, hu, hv, ht, sshn_t, sshn_u, sshn_v, *limits)
        r = D.psy.tracer_courant(RDT, *F, face_limit=limits[0], outflow_limit=limits[1])
        got = (r.face_max, r.outflow_max, (r.face_at[2] - 1) * g.nx + r.face_at[1] - 1,
               (r.outflow_at[2] - 1) * g.nx + r.outflow_at[1] - 1, r.face_over, r.outflow_over, r.invalid, r.wet)
        assert CN.same_record(got, want), (got, want)
        assert _line(what, got) in lines, (_line(what, got), lines)
        assert 0 < want.face_over < want.wet and want.invalid == 0
    assert "G: ranks 1 1" in lines
    assert r.face_at[0] == 1 and r.outflow_at[0] == 1
