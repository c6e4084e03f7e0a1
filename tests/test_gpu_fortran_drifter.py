"""GPU test (-m gpu): the Fortran drifter wrappers through a small program
(tests/fortran/ftest_drifter.f90, built by the Fortran layer's Makefile like every program there).  On the 26 x 22 grid of
tests/drifter_cases.py as grid_init makes it, drifters_create / drifter_step / drifters_get from Fortran must print the hashes
of the positions and statuses the Python wrapper leaves on the same hashed flow and the same particles -- after a call with
nsub = 1, after one more with nsub = 3 and after the particles were put again without a status array -- and those arrays
equal tests/drifter_numpy.py bit for bit; an argument out of order in the bind(C) interfaces or the wrappers shows up there."""
import os
import subprocess

import numpy as np
import pytest

import drifter_cases as DC
import drifter_numpy as DN
from conftest import ROOT

pytestmark = pytest.mark.gpu
FDIR = os.path.join(ROOT, "dl_esm_inf_amd", "fortran")
EXE = os.path.join(FDIR, "build", "ftest_drifter.exe")
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
    """the program's hash: h = rotl(h, 5) ^ bits over the elements in order (an int32 sign-extended to 64 bits)"""
    a = np.ascontiguousarray(a)
    bits = a.view(np.uint64) if a.dtype == np.float64 else a.astype(np.int64).view(np.uint64)
    h = 0
    for b in bits.tolist():
        h = (((h << 5) | (h >> 59)) & MASK64) ^ b
    return "%016X" % h


def _line(what, px, py, st):
    return "G: %s hashes %s %s %s counts %s" % (what, _hash(px), _hash(py), _hash(st),
                                                " ".join(str(int((st == s).sum())) for s in range(4)))


@pytest.mark.parametrize("n,alignment", [(1000, 2), (65, 1)])
def test_fortran_wrappers_print_the_python_wrappers_hashes(n, alignment):
    p = _run(n, alignment=alignment)
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
        g.decompose(23, 19)
        it = g.subdomain.internal
        user = np.ones((it.ystop + 1, it.xstop + 1), dtype=np.int32)
        user[:, 23:] = -1
        user[:, 0] = 0
        user[0, :] = 0
        user[-1, :] = 0
        user[DC.ISLAND] = 0
        user[DC.ROCK] = 0
        D.grid_init(g, 1000.0, 1000.0, tmask=user)
    finally:
        os.environ.pop("DL_ESM_ALIGNMENT", None)
    assert f"G: extents {g.nx} {g.ny}" in lines, lines
    assert (g.nx, g.ny) == (DC.LD, DC.NY)
    F, H = [], []
    for seed, pt in ((617, D.GO_U_POINTS), (618, D.GO_V_POINTS)):
        f = D.r2d_field(g, pt)
        D.psy.hash_init(f, seed)
        d = 3.0 * f.get_data() - 1.5
        f.set_data(d)
        F.append(f)
        H.append(np.ascontiguousarray(d))
    p1 = np.arange(n)
    px = 0.5 + 0.125 * ((37 * p1) % 211)
    py = 0.5 + 0.0625 * ((101 * p1) % 353)
    st = np.where((p1 + 1) % 11 == 0, 1 + (p1 + 1) % 3, 0).astype(np.int32)
    tm = g.tmask_device.cpu().numpy()
    dx, dy = g.dx_t_device.cpu().numpy(), g.dy_t_device.cpu().numpy()
    box = D.field_mod.field_bounds(g, D.GO_T_POINTS)[0].box()
    assert tuple(box) == (2, 24, 2, 20) and (tm[1:-2, 23] < 0).all() and tm[14, 16] == 0
    want = [px.copy(), py.copy(), st.copy()]
    dev = [torch.from_numpy(a.copy()).cuda() for a in want]

    def compare(what):
        torch.cuda.synchronize()
        got = [t.cpu().numpy() for t in dev]
        assert DN.same(got[0], want[0]) and DN.same(got[1], want[1]) and (got[2] == want[2]).all(), what
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        assert _line(what, *got) in lines, (what, _line(what, *got), lines)
        return got

    D.psy.drifter_step(400.0, *dev, *F, nsub=1)
    DN.drifter_step(400.0, 1, box, tm, dx, dy, *H, *want)
    one = compare("one")
    D.psy.drifter_step(400.0, *dev, *F, nsub=3)
    DN.drifter_step(400.0, 3, box, tm, dx, dy, *H, *want)
    three = compare("three")
    assert not DN.same(one[0], three[0])
    idle = st != 0
    assert idle.sum() == n // 11 and DN.same(three[0][idle], px[idle]) and (three[2][idle] == st[idle]).all()
    if n >= 1000:
        assert set(three[2].tolist()) == {0, 1, 2, 3}
    dev[2].zero_()
    want[2][:] = 0
    D.psy.drifter_step(400.0, *dev, *F, nsub=2)
    DN.drifter_step(400.0, 2, box, tm, dx, dy, *H, *want)
    compare("again")
