"""GPU test (-m gpu): the Fortran wrapper of the model's output fields through a small program
(tests/fortran/ftest_flow_output.f90, built by the Fortran layer's Makefile like every program there).  On a grid with a
-1/0/1 user tmask, flow_output from Fortran must print, for each of the six outputs, the hash of the array the Python wrapper
leaves on the same hashed inputs -- after one call that stores, after two more that add with weight 0.375 and after one that
stores the velocities alone; an argument out of order in the bind(C) interface or the wrapper shows up there -- and those
arrays equal tests/flow_output_numpy.py bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import flow_output_cases as OC
import flow_output_numpy as ON
from conftest import ROOT

pytestmark = pytest.mark.gpu
FDIR = os.path.join(ROOT, "dl_esm_inf_amd", "fortran")
EXE = os.path.join(FDIR, "build", "ftest_flow_output.exe")
MASK64 = (1 << 64) - 1


def _run(*args, alignment=None):
    subprocess.check_call(["make", "-C", FDIR], stdout=subprocess.DEVNULL)
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "DL_ESM_ALIGNMENT"):
        env.pop(k, None)
    if alignment:
        env["DL_ESM_ALIGNMENT"] = str(alignment)
    return subprocess.run(["timeout", "-k", "10", "120", EXE, *map(str, args)], env=env, capture_output=True, text=True)


def _hash(a):
    """the program's hash: h = rotl(h, 5) ^ bits over the cells in memory order"""
    h = 0
    for bits in np.ascontiguousarray(a).view(np.uint64).ravel().tolist():
        h = (((h << 5) | (h >> 59)) & MASK64) ^ bits
    return "%016X" % h


def _line(what, arrays):
    return "G: %s hashes %s" % (what, " ".join(_hash(a) for a in arrays))


@pytest.mark.parametrize("nx,ny,alignment", [(257, 6, 2), (128, 4, 1)])
def test_fortran_wrapper_prints_the_python_wrappers_hashes(nx, ny, alignment):
    """array shapes (260, 9) -- the tile, three waves a row -- and (131, 7) -- an odd pitch, the general path"""
    p = _run(nx, ny, alignment=alignment)
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
    out = []
    for _ in range(ON.COUNT):
        f = D.r2d_field(g, T)
        f.set_data(np.full((g.ny, g.nx), OC.SENTINEL))
        out.append(f)
    named = dict(zip(ON.NAMES, out))
    tm = g.tmask_device.cpu().numpy()
    dx_v, dy_u = g.dx_v_device.cpu().numpy(), g.dy_u_device.cpu().numpy()
    box = F[3].internal.box()
    want = OC.outputs(tm.shape, OC.ALL)

    def compare(what):
        got = [f.get_data() for f in out]
        for k in range(ON.COUNT):
            assert ON.same(got[k], want[k]) and np.isfinite(got[k]).all(), (what, ON.NAMES[k])
        assert _line(what, got) in lines, (what, _line(what, got), lines)
        return got

    D.psy.flow_output(*F, **named)
    ON.flow_output(ON.SET, 0.0, box, tm, dx_v, dy_u, *H, want)
    first = compare("set")
    for _ in range(2):
        D.psy.flow_output(*F, **named, weight=0.375)
        ON.flow_output(ON.ADD, 0.375, box, tm, dx_v, dy_u, *H, want)
    second = compare("add")
    D.psy.flow_output(*F, ut=out[ON.UT], vt=out[ON.VT], speed=out[ON.SPEED])
    ON.flow_output(ON.SET, 0.0, box, tm, None, None, H[0], H[1], None, None, [None, *want[1:4], None, None])
    third = compare("uvs")
    w = ON.written(tm, box, ON.VORT)
    assert w.sum() < ON.written(tm, box, ON.UT).sum() and (first[ON.VORT][~w] == OC.SENTINEL).all()
    assert w.sum() >= 10 or ny < 6                                   # (the four-row grid holds no corner clear of land)
    # six different fields, and the sums differ from them wherever a cell is written
    assert len({_hash(a) for a in first + second}) == (12 if w.any() else 11)
    for k in range(1, ON.COUNT):
        assert ON.same(third[k], first[k]) == (k in (ON.UT, ON.VT, ON.SPEED) or (k == ON.VORT and not w.any())), ON.NAMES[k]
