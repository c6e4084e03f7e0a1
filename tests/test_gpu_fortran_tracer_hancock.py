"""GPU test (-m gpu): the Fortran wrappers of time-centred limited tracer transport through a small
program (tests/fortran/ftest_tracer_hancock.f90, built by the Fortran layer's Makefile like every program there).  On a grid with
a -1/0/1 user tmask, invoke_tracer_step_hancock of two tracers from Fortran must leave the bits the Python wrapper leaves on the
same inputs -- the same field_checksum and the same field_stats, without and with the grid's mask (an argument out of order in
the bind(C) interface or the wrapper shows up there) -- and the Python wrapper's result equals tests/tracer_hancock_numpy.py in
every cell.  The same through invoke_tracer_step_hancock_dm on a one-rank grid decomposed with halo_width = 2.  On a halo_width = 1
grid the distributed wrapper must stop, and on a decomposed grid the single-domain one.  rdt = 1.0e7 on the 1000 m grid puts
faces on both sides of a Courant number of 1 (asserted on the host)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import tracer_hancock_numpy as TH
import tracer_numpy as TN
from conftest import ROOT

pytestmark = pytest.mark.gpu
FDIR = os.path.join(ROOT, "dl_esm_inf_amd", "fortran")
EXE = os.path.join(FDIR, "build", "ftest_tracer_hancock.exe")


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


def _stats_line(st):
    return " ".join([_bits(st.min), _bits(st.max), _bits(st.sum), _bits(st.sumsq), str(int(st.count)), str(int(st.nonfinite))])


@pytest.mark.parametrize("nx,ny,alignment,mode", [(257, 6, 2, "run"), (128, 4, 1, "run"), (254, 5, 2, "dm")])
def test_fortran_wrappers_leave_the_python_wrappers_bits(nx, ny, alignment, mode):
    """array shapes (260, 9) -- the tile, three waves a row -- and (131, 7) -- an odd pitch, the general path; "dm": (260, 10)
    on a grid decomposed with halo_width = 2, the distributed wrapper over a plan without messages"""
    p = _run(nx, ny, mode, alignment=alignment)
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
        g.decompose(nx, ny, halo_width=2 if mode == "dm" else 1)
        it = g.subdomain.internal
        jj, ii = np.mgrid[1:it.ystop + 2, 1:it.xstop + 2]
        user = ((7 * ii + 13 * jj + (ii * jj) // 5) % 3 - 1).astype(np.int32)
        user[:3, :3] = 0
        D.grid_init(g, 1000.0, 1000.0, tmask=user)
    finally:
        os.environ.pop("DL_ESM_ALIGNMENT", None)
    assert f"G: extents {g.nx} {g.ny}" in lines, lines
    assert (g.nx, g.ny) == ((260, 10) if mode == "dm" else (nx + 3, ny + 3))
    T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
    F, H = [], []
    for k, pt in enumerate((T, U, V, T, U, V, T, U, V), start=1):           # ssha un vn ht hu hv sshn_t sshn_u sshn_v
        f = D.r2d_field(g, pt)
        D.psy.hash_init(f, 500 + k)
        d = f.get_data()
        d = 0.4 * d - 0.2 if k in (2, 3) else 10.0 + d if k in (4, 5, 6) else 0.05 * d
        f.set_data(d)
        F.append(f)
        H.append(np.ascontiguousarray(d))
    Ci, Co, c_in = [], [], []
    for k in (1, 2):
        f, o = D.r2d_field(g, T), D.r2d_field(g, T)
        D.psy.hash_init(f, 600 + k)
        d = float(k) + f.get_data()
        f.set_data(d)
        o.set_data(np.full((g.ny, g.nx), -7.0))
        Ci.append(f)
        Co.append(o)
        c_in.append(np.ascontiguousarray(d))
    (D.psy.invoke_tracer_step_hancock_dm if mode == "dm" else D.psy.invoke_tracer_step_hancock)(1.0e7, Co, Ci, *F)
    torch.cuda.synchronize()
    tm = g.tmask_device.cpu().numpy()
    want = [np.full((g.ny, g.nx), -7.0) for _ in range(2)]
    ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v = H
    TH.tracer_step_hancock(1.0e7, Co[0].internal.box(), tm, g.area_t_device.cpu().numpy(), un, vn, hu, hv, ht, sshn_t, sshn_u,
                         sshn_v, ssha, c_in, want)
    mid, big = TH.face_shares(1.0e7, Co[0].internal.box(), tm, g.area_t_device.cpu().numpy(), un, vn, hu, hv, ht, sshn_t, sshn_u,
                              sshn_v)
    assert mid >= 0.10 and big >= 0.10, (mid, big)
    for k in range(2):
        got = Co[k].get_data()
        assert TN.same(got, want[k]), k
        assert (got != -7.0).any() and (got[1:-1, 1:-1] == -7.0).any()
        st = D.field_stats([Co[k]])[0]
        stm = D.field_stats([Co[k]], masks=g.tmask_device)[0]
        assert f"G: tracer {k + 1} checksum {_bits(D.field_checksum(Co[k]))}" in lines, lines
        assert f"G: tracer {k + 1} stats {_stats_line(st)}" in lines, lines
        assert f"G: tracer {k + 1} wet stats {_stats_line(stm)}" in lines, lines
        xs, xe, ys, ye = Co[k].internal.box()
        assert stm.nonfinite == 0 and stm.count == int((tm[ys - 1:ye, xs - 1:xe] > 0).sum())


@pytest.mark.parametrize("mode,word", [("decomposed", "invoke_tracer_step_hancock_dm"), ("hw1", "halo_width = 2")])
def test_fortran_wrappers_stop(mode, word):
    p = _run(64, 32, mode, alignment=64)
    assert p.returncode not in (0, 124, 137), p.stdout[-2000:]
    assert word in (p.stdout + p.stderr).replace("\n ", ""), (p.stdout[-2000:], p.stderr[-2000:])
    assert "G: ran where the wrapper must stop" not in p.stdout
