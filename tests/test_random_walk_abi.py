"""CPU tests of the boundary of the random walk in a varying diffusivity: the two entries are exported
from the product and from the lab build and stand in the header, the ctypes table, INTEGRATION.md and dlesm_hip_mod with one
argument list each; no other exported name contains `random_walk`, and theirs contain none of `dispersal`, `drifter`,
`particle`, `cell_bin`, `migrate` (the ABI tests of sections 6.17 to 6.21 pin those sets); the Python and Fortran names are
public; dlesm_version() is unchanged; without a GPU the entries return DLESM_ENODEV and write nothing, and with one every
refusal is DLESM_EINVAL with nothing written."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

import dl_esm_inf_amd as D
from dl_esm_inf_amd import _cabi

L = _cabi.lib()
_i, _d, _vp, _ll = C.c_int, C.c_double, C.c_void_p, C.c_longlong
_GRID = ["int ld", "int ny", "int xstart", "int xstop", "int ystart", "int ystop", "const int *tmask", "const double *dx_t",
         "const double *dy_t", "const double *un", "const double *vn"]
_RNG = ["double h", "int nsub", "const double *kh_t", "long long seed", "long long tick", "const long long *tick_dev"]
ENTRIES = {
    "dlesm_random_walk_f64": (
        _RNG + _GRID + ["long long n", "const int *id", "double *px", "double *py", "int *status", "void *stream"],
        [_d, _i, _vp, _ll, _ll, _vp] + [_i] * 6 + [_vp] * 5 + [_ll] + [_vp] * 5),
    "dlesm_random_walk_set": (
        ["dlesm_drifters *set"] + _RNG + _GRID + ["void *stream"],
        [_vp, _d, _i, _vp, _ll, _ll, _vp] + [_i] * 6 + [_vp] * 6),
}


def _names(args):
    return [a.split()[-1].lstrip("*") for a in args]


def test_header_exports_ctypes_and_documents_agree():
    raw = open(os.path.join(ROOT, "include", "dlesm_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    fortran = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_hip_mod.f90")).read()
    exported = []
    for lib in [_cabi.LIB_PATH, os.path.join(os.path.dirname(_cabi.LIB_PATH), "libdlesm_hip_lab.so")]:
        out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
        exported.append({l.split()[-1] for l in out.splitlines() if " T " in l})
    for entry, (args, ctypes_args) in ENTRIES.items():
        assert entry in exported[0] and entry in exported[1], entry
        assert not any(word in entry for word in ("dispersal", "drifter", "particle", "cell_bin", "migrate")), entry
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % entry, txt)
        assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == args, entry
        res, got = _cabi.PROTOTYPES[entry]
        assert res is C.c_int and list(got) == ctypes_args, entry
        m = re.search(r"`%s\(([^)]*)\)`" % entry, doc)
        assert m and [a.strip() for a in m.group(1).replace("\n", " ").split(",")] == _names(args), entry
        m = re.search(r"function %s\((.*?)\)\s*bind\(C, name=\"%s\"\)" % (entry, entry), fortran, flags=re.S)
        assert m and [a.strip() for a in m.group(1).replace("&", " ").split(",")] == _names(args), entry
    for names in exported:
        assert {e for e in names if "random_walk" in e} == set(ENTRIES)
    for name in ("psy.random_walk", "call random_walk("):
        assert name in doc, name
    assert "section 6.22" in raw
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 6.22 " in design and all(e in design for e in ENTRIES)
    assert "dlesm_random_walk_f64" in open(os.path.join(ROOT, "README.md")).read()
    assert L.dlesm_version() == 310


def test_the_wrappers_are_public():
    from dl_esm_inf_amd import psy
    assert D.random_walk is psy.random_walk
    sig = inspect.signature(psy.random_walk).parameters
    assert list(sig) == ["h", "kh_t", "seed", "tick", "px", "py", "status", "un", "vn", "nsub", "ids", "tick_dev", "stream"]
    assert sig["nsub"].default == 1 and all(sig[k].default is None for k in ("ids", "tick_dev", "stream"))
    assert "On a decomposed grid kh_t needs valid depth-1 halos" in " ".join(psy.random_walk.__doc__.split())
    psy_f = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_psy_mod.f90")).read()
    assert re.search(r"public ::[^\n]*\brandom_walk\b", psy_f)
    assert re.search(r"subroutine random_walk\(set, h, nsub, kh_t, seed, tick, un, vn\)", psy_f)
    body = psy_f[psy_f.index("subroutine random_walk("):psy_f.index("end subroutine random_walk")]
    assert re.search(r"type\(r2d_field\), intent\(inout\), target :: kh_t", body)
    assert re.search(r"integer\(c_long_long\), intent\(in\) :: seed, tick", body)
    assert "dlesm_random_walk_set(" in body


def test_without_a_gpu_the_entries_fail_loudly_and_write_nothing():
    """DLESM_ENODEV without a device; with one, host arrays of a valid shape pass every check that needs no device and each
    refusal is DLESM_EINVAL"""
    a = np.ones((8, 8))
    kh = np.full((8, 8), 2.0)
    t = np.ones((8, 8), dtype=np.int32)
    px, py, st = np.full(4, 3.5), np.full(4, 4.5), np.zeros(4, dtype=np.int32)
    ids = np.arange(8, dtype=np.int32)
    tk = np.full(2, 5, dtype=np.int64)
    have_gpu = L.dlesm_device_count() > 0
    want = _cabi.EINVAL if have_gpu else _cabi.ENODEV
    fields = [a.ctypes.data] * 4

    def step(h=10.0, nsub=1, kh_t=kh.ctypes.data, seed=-3, tick=0, tick_dev=tk.ctypes.data, tmask=t.ctypes.data, n=4,
             id_=ids.ctypes.data, x=px.ctypes.data, s=st.ctypes.data):
        return L.dlesm_random_walk_f64(h, nsub, kh_t, seed, tick, tick_dev, 8, 8, 2, 7, 2, 7, tmask, *fields, n, id_, x,
                                       py.ctypes.data, s, None)

    assert step(tmask=None) == want
    if not have_gpu:
        assert b"no HIP device" in L.dlesm_last_error()
    # what dlesm_drifter_step_f64 refuses
    assert step(nsub=0) == want and step(nsub=1025) == want and step(h=float("nan")) == want and step(n=-1) == want
    assert step(x=None) == want and step(x=py.ctypes.data) == want
    # the rules of tick, id and tick_dev
    assert step(tick=-1) == want and step(tick=2 ** 63 - 1) == want and step(tick=2 ** 63 - 3, nsub=3) == want
    assert step(id_=ids.ctypes.data + 2) == want and step(tick_dev=tk.ctypes.data + 4) == want
    if have_gpu:
        assert b"tick_dev is not 8-byte aligned" in L.dlesm_last_error()
    assert step(id_=px.ctypes.data) == want and step(id_=py.ctypes.data + 16) == want and step(id_=st.ctypes.data) == want
    assert step(tick_dev=px.ctypes.data + 8) == want and step(tick_dev=py.ctypes.data) == want
    assert step(tick_dev=st.ctypes.data + 8) == want
    assert step(tick_dev=t.ctypes.data + 8) == want and step(tick_dev=a.ctypes.data + 504) == want
    assert step(tick_dev=ids.ctypes.data + 8) == want
    # the entry's own refusals
    assert step(kh_t=None) == want
    if have_gpu:
        assert b"null kh_t" in L.dlesm_last_error()
    assert step(kh_t=kh.ctypes.data + 4) == want
    if have_gpu:
        assert b"kh_t is not 8-byte aligned" in L.dlesm_last_error()
    assert step(kh_t=px.ctypes.data) == want and step(kh_t=py.ctypes.data - 504) == want and step(kh_t=st.ctypes.data) == want
    assert step(tick_dev=kh.ctypes.data) == want and step(tick_dev=kh.ctypes.data + 504) == want
    if have_gpu:
        assert b"overlaps the input kh_t" in L.dlesm_last_error()
    handle = C.c_void_p(0x1234)
    assert L.dlesm_random_walk_set(None, 10.0, 1, kh.ctypes.data, 7, 0, None, 8, 8, 2, 7, 2, 7, t.ctypes.data, *fields, None) == want
    if not have_gpu:
        assert L.dlesm_random_walk_set(handle, 10.0, 1, kh.ctypes.data, 7, 0, None, 8, 8, 2, 7, 2, 7, t.ctypes.data, *fields,
                                       None) == _cabi.ENODEV
    assert (px == 3.5).all() and (py == 4.5).all() and (st == 0).all() and (a == 1.0).all() and (t == 1).all()
    assert (tk == 5).all() and (ids == np.arange(8)).all() and (kh == 2.0).all()
