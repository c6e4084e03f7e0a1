"""GPU test (-m gpu): the Fortran wrappers of the coupled step on a decomposed grid through a small
program (tests/fortran/ftest_coupled_step.f90, built by the Fortran layer's Makefile like every program there).  On a one-rank
grid decomposed with halo_width = 2, with a -1/0/1 user tmask, one closed-basin invoke_nemolite_coupled_step_dm with the Hancock
scheme and two tracers from Fortran must leave the bits the Python wrappers invoke_nemolite_step followed by
invoke_tracer_step_hancock leave on the same inputs -- the same field_checksum and the same field_stats of all five flow
outputs and both tracers (an argument out of order in the bind(C) interface or the wrapper shows up there) -- and
exchange_mask_halos must leave the mask as it was.  On a halo_width = 1 grid the wrapper must stop for the MUSCL scheme and name
halo_width = 2."""
import os
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
FDIR = os.path.join(ROOT, "dl_esm_inf_amd", "fortran")
EXE = os.path.join(FDIR, "build", "ftest_coupled_step.exe")
OUTS = ("ssha", "ssha_u", "ssha_v", "ua", "va")


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


@pytest.mark.parametrize("nx,ny,alignment,shape", [(254, 5, 2, (260, 10)), (126, 4, 1, (131, 9))])
def test_fortran_wrapper_leaves_the_python_wrappers_bits(nx, ny, alignment, shape):
    """array shapes (260, 10) -- the one-sweep step and the wave-tile tracer sweep -- and (131, 9), an odd pitch: the five
    entries and the one-cell-per-thread tracer kernel"""
    p = _run(nx, ny, "dm", alignment=alignment)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    lines = [l.strip() for l in p.stdout.splitlines() if l.startswith("G:")]
    print("\n".join(lines))
    assert "G: the mask is unchanged" in lines, lines

    import torch
    import dl_esm_inf_amd as D
    torch.cuda.set_device(0)
    D.parallel_init(0, 1)
    os.environ["DL_ESM_ALIGNMENT"] = str(alignment)
    try:
        g = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
        g.decompose(nx, ny, halo_width=2)
        it = g.subdomain.internal
        jj, ii = np.mgrid[1:it.ystop + 2, 1:it.xstop + 2]
        user = ((7 * ii + 13 * jj + (ii * jj) // 5) % 3 - 1).astype(np.int32)
        user[:3, :3] = 0
        D.grid_init(g, 1000.0, 1000.0, tmask=user)
    finally:
        os.environ.pop("DL_ESM_ALIGNMENT", None)
    assert f"G: extents {g.nx} {g.ny}" in lines, lines
    assert (g.nx, g.ny) == shape
    D.psy.coriolis(g)
    T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
    F = []
    # ssha ssha_u ssha_v ua va un vn ht hu hv sshn_t sshn_u sshn_v
    for k, pt in enumerate((T, U, V, U, V, U, V, T, U, V, T, U, V), start=1):
        f = D.r2d_field(g, pt)
        D.psy.hash_init(f, 900 + k)
        d = f.get_data()
        if k in (8, 9, 10):
            d = 10.0 + d
        elif k == 1:
            d = 1000.0 + d
        elif k in (2, 3, 4, 5):
            d = np.full_like(d, -7.0)
        elif k in (6, 7):
            d = 0.4 * d - 0.2
        else:
            d = 0.05 * d
        f.set_data(d)
        F.append(f)
    Ci, Co = [], []
    for k in (1, 2):
        f, o = D.r2d_field(g, T), D.r2d_field(g, T)
        D.psy.hash_init(f, 600 + k)
        f.set_data(float(k) + f.get_data())
        o.set_data(np.full((g.ny, g.nx), -7.0))
        Ci.append(f)
        Co.append(o)
    prm = D.psy.momentum_params(20.0, 0.00015, 50.0, 9.80665)
    D.psy.invoke_nemolite_step(prm, *F)
    ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v = F[0], *F[5:]
    D.psy.invoke_tracer_step_hancock(prm.rdt, Co, Ci, ssha, un, vn, ht, hu, hv, sshn_t, sshn_u, sshn_v)
    torch.cuda.synchronize()
    for name, f in list(zip(OUTS, F[:5])) + [("c1", Co[0]), ("c2", Co[1])]:
        if name != "ssha":
            got = f.get_data()
            assert (got != -7.0).any() and (got == -7.0).any(), name
        st = D.field_stats([f])[0]
        assert f"G: {name} checksum {_bits(D.field_checksum(f))}" in lines, (name, lines)
        assert f"G: {name} stats {_stats_line(st)}" in lines, (name, lines)


def test_fortran_wrapper_stops_on_halo_width_1_with_a_limited_scheme():
    p = _run(64, 32, "hw1", alignment=64)
    assert p.returncode not in (0, 124, 137), p.stdout[-2000:]
    assert "halo_width = 2" in (p.stdout + p.stderr).replace("\n ", ""), (p.stdout[-2000:], p.stderr[-2000:])
    assert "G: ran where the wrapper must stop" not in p.stdout
