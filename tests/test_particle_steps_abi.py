"""CPU tests of the boundary of the particle steps -- the drifters, the dispersal step (6.20) and the
random walk in a varying diffusivity (6.22): each family's entries are exported from the product and from the lab build and
stand in the header, the ctypes table, INTEGRATION.md and dlesm_hip_mod with one argument list each; no other exported name
contains the family's word, and the entries of 6.20 and 6.22 contain none of the earlier families' words (the ABI tests of
sections 6.18, 6.19 and 6.21 pin those sets); the DLESM_DRIFTER_* numbers are the same in the header, the ctypes module, the
Fortran module and the restatement; the Python and Fortran names are public; dlesm_version() is unchanged; without a GPU the
entries return DLESM_ENODEV and write nothing, and with one every refusal is DLESM_EINVAL with nothing written."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import dl_esm_inf_amd as D
from dl_esm_inf_amd import _cabi

import drifter_numpy as DN

L = _cabi.lib()
_i, _d, _vp, _ll = C.c_int, C.c_double, C.c_void_p, C.c_longlong
_GRID = ["int ld", "int ny", "int xstart", "int xstop", "int ystart", "int ystop", "const int *tmask", "const double *dx_t",
         "const double *dy_t", "const double *un", "const double *vn"]
_ARRAYS = ["long long n", "const int *id", "double *px", "double *py", "int *status", "void *stream"]
_RNG = {"dispersal": ["double h", "int nsub", "double kh", "long long seed", "long long tick", "const long long *tick_dev"],
        "random_walk": ["double h", "int nsub", "const double *kh_t", "long long seed", "long long tick", "const long long *tick_dev"]}
ENTRIES = {
    "drifter": {
        "dlesm_drifter_step_f64": (
            ["double h", "int nsub"] + _GRID + ["long long n", "double *px", "double *py", "int *status", "void *stream"],
            [_d] + [_i] * 7 + [_vp] * 5 + [_ll] + [_vp] * 4),
        "dlesm_drifter_sample_f64": (
            ["int ld", "int ny", "int xstart", "int xstop", "int ystart", "int ystop", "long long n", "const double *px",
             "const double *py", "const int *status", "const double *const *fields", "double *const *out", "int nfields",
             "void *stream"],
            [_i] * 6 + [_ll] + [_vp] * 3 + [C.POINTER(_vp), C.POINTER(_vp), _i, _vp]),
        "dlesm_drifters_create": (["long long n", "dlesm_drifters **set"], [_ll, C.POINTER(_vp)]),
        "dlesm_drifters_put": (["dlesm_drifters *set", "const double *px", "const double *py", "const int *status"], [_vp] * 4),
        "dlesm_drifters_get": (["dlesm_drifters *set", "double *px", "double *py", "int *status"], [_vp] * 4),
        "dlesm_drifters_arrays": (["dlesm_drifters *set", "long long *n", "double **px", "double **py", "int **status"],
                                  [_vp, C.POINTER(_ll), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
        "dlesm_drifters_destroy": (["dlesm_drifters *set"], [_vp]),
    },
    "dispersal": {
        "dlesm_dispersal_step_f64": (_RNG["dispersal"] + _GRID + _ARRAYS,
                                     [_d, _i, _d, _ll, _ll, _vp] + [_i] * 6 + [_vp] * 5 + [_ll] + [_vp] * 5),
        "dlesm_dispersal_step_set": (["dlesm_drifters *set"] + _RNG["dispersal"] + _GRID + ["void *stream"],
                                     [_vp, _d, _i, _d, _ll, _ll, _vp] + [_i] * 6 + [_vp] * 6),
    },
    "random_walk": {
        "dlesm_random_walk_f64": (_RNG["random_walk"] + _GRID + _ARRAYS,
                                  [_d, _i, _vp, _ll, _ll, _vp] + [_i] * 6 + [_vp] * 5 + [_ll] + [_vp] * 5),
        "dlesm_random_walk_set": (["dlesm_drifters *set"] + _RNG["random_walk"] + _GRID + ["void *stream"],
                                  [_vp, _d, _i, _vp, _ll, _ll, _vp] + [_i] * 6 + [_vp] * 6),
    },
}
# family -> (words no entry's name contains, the libraries in which the family's word names its entries alone, what
# INTEGRATION.md names, what the header's raw text holds, the heading in DESIGN.md, whether README.md names the step)
FAMILIES = {
    "drifter": ((), 1,
                ("psy.drifter_step", "psy.drifter_sample", "call drifter_step(", "call drifters_create(", "call drifters_get(",
                 "call drifters_free(", "drifters_type", "DLESM_DRIFTER_ACTIVE", "DLESM_DRIFTER_LEFT", "DLESM_DRIFTER_OPEN",
                 "DLESM_DRIFTER_GROUNDED", "DLESM_DRIFTER_MAX_SUB", "DLESM_DRIFTER_MAX_FIELDS"),
                (), "### 6.17 Drifters (frozen here)", None),
    "dispersal": (("drifter", "particle", "cell_bin"), 2, ("psy.dispersal_step", "call dispersal_step("),
                  ("section 6.20", "REPLAYS THE SAME KICKS"),       # a graph without tick_dev: the header says so
                  "### 6.20 ", "dlesm_dispersal_step_f64"),
    "random_walk": (("dispersal", "drifter", "particle", "cell_bin", "migrate"), 2, ("psy.random_walk", "call random_walk("),
                    ("section 6.22",), "### 6.22 ", "dlesm_random_walk_f64"),
}


def _names(args):
    return [a.split()[-1].lstrip("*") for a in args]


@pytest.mark.parametrize("family", list(ENTRIES))
def test_header_exports_ctypes_and_documents_agree(family):
    entries = ENTRIES[family]
    foreign, nlibs, doc_names, raw_texts, heading, readme = FAMILIES[family]
    raw = open(os.path.join(ROOT, "include", "dlesm_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    fortran = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_hip_mod.f90")).read()
    exported = []
    for lib in [_cabi.LIB_PATH, os.path.join(os.path.dirname(_cabi.LIB_PATH), "libdlesm_hip_lab.so")]:
        out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
        exported.append({l.split()[-1] for l in out.splitlines() if " T " in l})
    for entry, (args, ctypes_args) in entries.items():
        assert entry in exported[0] and entry in exported[1], entry
        assert not any(word in entry for word in foreign), entry
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % entry, txt)
        assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == args, entry
        res, got = _cabi.PROTOTYPES[entry]
        assert res is C.c_int and list(got) == ctypes_args, entry
        m = re.search(r"`%s\(([^)]*)\)`" % entry, doc)
        assert m and [a.strip() for a in m.group(1).replace("\n", " ").split(",")] == _names(args), entry
        m = re.search(r"function %s\((.*?)\)\s*bind\(C, name=\"%s\"\)" % (entry, entry), fortran, flags=re.S)
        assert m and [a.strip() for a in m.group(1).replace("&", " ").split(",")] == _names(args), entry
    for names in exported[:nlibs]:
        assert {e for e in names if family in e} == set(entries)
    for name in doc_names:
        assert name in doc, name
    for text in raw_texts:
        assert text in raw, text
    if family == "drifter":
        assert re.search(r"typedef struct dlesm_drifters dlesm_drifters;", txt)
        assert raw.count("section 6.17") >= 2                        # the entries' comment and the owner's
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert heading in design and all(e in design for e in entries)
    assert readme is None or readme in open(os.path.join(ROOT, "README.md")).read()
    assert L.dlesm_version() == 310


def test_the_status_numbers_agree():
    h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dlesm_hip.h")).read(), flags=re.S)
    assert re.search(r"enum\s*\{\s*DLESM_DRIFTER_ACTIVE = 0,\s*DLESM_DRIFTER_LEFT,\s*DLESM_DRIFTER_OPEN,\s*"
                     r"DLESM_DRIFTER_GROUNDED\s*\}", h)
    assert re.search(r"enum\s*\{\s*DLESM_DRIFTER_MAX_SUB = 1024,\s*DLESM_DRIFTER_MAX_FIELDS = 8\s*\}", h)
    ours = (_cabi.DRIFTER_ACTIVE, _cabi.DRIFTER_LEFT, _cabi.DRIFTER_OPEN, _cabi.DRIFTER_GROUNDED)
    assert ours == (DN.ACTIVE, DN.LEFT, DN.OPEN, DN.GROUNDED) == (0, 1, 2, 3)
    assert (_cabi.DRIFTER_MAX_SUB, _cabi.DRIFTER_MAX_FIELDS) == (DN.MAX_SUB, DN.MAX_FIELDS) == (1024, 8)
    fortran = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_hip_mod.f90")).read()
    m = re.search(r"DLESM_DRIFTER_ACTIVE = (\d), DLESM_DRIFTER_LEFT = (\d), DLESM_DRIFTER_OPEN = (\d), &\s*"
                  r"DLESM_DRIFTER_GROUNDED = (\d)", fortran)
    assert m and tuple(map(int, m.groups())) == ours


def test_the_drifter_wrappers_are_public():
    from dl_esm_inf_amd import psy
    assert D.drifter_step is psy.drifter_step and D.drifter_sample is psy.drifter_sample
    sig = inspect.signature(psy.drifter_step).parameters
    assert list(sig) == ["h", "px", "py", "status", "un", "vn", "nsub", "stream"]
    assert sig["nsub"].default == 1 and sig["stream"].default is None
    sig = inspect.signature(psy.drifter_sample).parameters
    assert list(sig) == ["px", "py", "status", "fields", "out", "stream"] and sig["out"].default is None
    psy_f = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_psy_mod.f90")).read()
    for name in ("drifters_type", "drifters_create", "drifters_get", "drifters_free", "drifter_step"):
        assert re.search(r"public ::[^\n]*\b%s\b" % name, psy_f), name
    for name, args in (("drifters_create", "set, px, py, status"), ("drifters_get", "set, px, py, status"),
                       ("drifters_free", "set"), ("drifter_step", "set, h, nsub, un, vn")):
        assert re.search(r"subroutine %s\(%s\)" % (name, re.escape(args)), psy_f), name
    assert "drifter_sample" not in psy_f                              # no sampling wrapper in Fortran


@pytest.mark.parametrize("name, third", [("dispersal_step", "kh"), ("random_walk", "kh_t")])
def test_the_random_wrappers_are_public(name, third):
    from dl_esm_inf_amd import psy
    assert getattr(D, name) is getattr(psy, name)
    sig = inspect.signature(getattr(psy, name)).parameters
    assert list(sig) == ["h", third, "seed", "tick", "px", "py", "status", "un", "vn", "nsub", "ids", "tick_dev", "stream"]
    assert sig["nsub"].default == 1 and all(sig[k].default is None for k in ("ids", "tick_dev", "stream"))
    psy_f = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_psy_mod.f90")).read()
    assert re.search(r"public ::[^\n]*\b%s\b" % name, psy_f)
    assert re.search(r"subroutine %s\(set, h, nsub, %s, seed, tick, un, vn\)" % (name, third), psy_f)
    body = psy_f[psy_f.index("subroutine %s(" % name):psy_f.index("end subroutine %s" % name)]
    assert re.search(r"integer\(c_long_long\), intent\(in\) :: seed, tick", body)
    if name == "dispersal_step":
        assert "dlesm_dispersal_step_set(" in body and "drifter_sample" not in psy_f
    else:
        assert "On a decomposed grid kh_t needs valid depth-1 halos" in " ".join(psy.random_walk.__doc__.split())
        assert re.search(r"type\(r2d_field\), intent\(inout\), target :: kh_t", body)
        assert "dlesm_random_walk_set(" in body


def test_without_a_gpu_the_drifter_entries_fail_loudly_and_write_nothing():
    """DLESM_ENODEV without a device; with one, host arrays of a valid shape pass every check that needs no device and the
    bad arguments are refused"""
    a = np.ones((8, 8))
    t = np.ones((8, 8), dtype=np.int32)
    px, py, st = np.full(4, 3.5), np.full(4, 4.5), np.zeros(4, dtype=np.int32)
    o = np.full(4, -7.0)
    have_gpu = L.dlesm_device_count() > 0
    want = _cabi.EINVAL if have_gpu else _cabi.ENODEV
    fields = [a.ctypes.data] * 4

    def step(h=10.0, nsub=1, tmask=t.ctypes.data, n=4, x=px.ctypes.data):
        return L.dlesm_drifter_step_f64(h, nsub, 8, 8, 2, 7, 2, 7, tmask, *fields, n, x, py.ctypes.data, st.ctypes.data, None)

    assert step(tmask=None) == want
    if not have_gpu:
        assert b"no HIP device" in L.dlesm_last_error()
    assert step(nsub=0) == want and step(nsub=1025) == want and step(h=float("nan")) == want and step(n=-1) == want
    assert step(x=None) == want and step(x=py.ctypes.data) == want
    pf, po = (C.c_void_p * 1)(a.ctypes.data), (C.c_void_p * 1)(o.ctypes.data)
    args = (8, 8, 2, 7, 2, 7, 4, px.ctypes.data, py.ctypes.data, st.ctypes.data)
    assert L.dlesm_drifter_sample_f64(*args, pf, po, 0, None) == want
    assert L.dlesm_drifter_sample_f64(*args, pf, po, 9, None) == want
    assert L.dlesm_drifter_sample_f64(*args, None, po, 1, None) == want
    assert L.dlesm_drifter_sample_f64(*args, pf, (C.c_void_p * 1)(), 1, None) == want
    handle = C.c_void_p(0x1234)
    if not have_gpu:
        assert L.dlesm_drifters_create(4, C.byref(handle)) == _cabi.ENODEV and b"no HIP device" in L.dlesm_last_error()
        assert handle.value == 0x1234
    assert L.dlesm_drifters_create(-1, C.byref(handle)) == want
    assert L.dlesm_drifters_put(None, px.ctypes.data, py.ctypes.data, None) == _cabi.EINVAL
    assert L.dlesm_drifters_get(None, px.ctypes.data, py.ctypes.data, st.ctypes.data) == _cabi.EINVAL
    assert L.dlesm_drifters_arrays(None, None, None, None, None) == _cabi.EINVAL
    assert L.dlesm_drifters_destroy(None) == 0
    assert (px == 3.5).all() and (py == 4.5).all() and (st == 0).all() and (o == -7.0).all() and (a == 1.0).all()


@pytest.mark.parametrize("family", ["dispersal", "random_walk"])
def test_without_a_gpu_the_random_entries_fail_loudly_and_write_nothing(family):
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
    walk = family == "random_walk"
    f64, set_ = (L.dlesm_random_walk_f64, L.dlesm_random_walk_set) if walk else (L.dlesm_dispersal_step_f64,
                                                                                   L.dlesm_dispersal_step_set)

    def step(h=10.0, nsub=1, k=kh.ctypes.data if walk else 1.0, seed=-3, tick=0, tick_dev=tk.ctypes.data, tmask=t.ctypes.data,
             n=4, id_=ids.ctypes.data, x=px.ctypes.data, s=st.ctypes.data):
        return f64(h, nsub, k, seed, tick, tick_dev, 8, 8, 2, 7, 2, 7, tmask, *fields, n, id_, x, py.ctypes.data, s, None)

    def own():
        if not walk:
            for k in (-1.0, -1e-300, float("nan"), float("inf"), float("-inf")):
                assert step(k=k) == want, k
            return
        assert step(k=None) == want
        if have_gpu:
            assert b"null kh_t" in L.dlesm_last_error()
        assert step(k=kh.ctypes.data + 4) == want
        if have_gpu:
            assert b"kh_t is not 8-byte aligned" in L.dlesm_last_error()
        assert step(k=px.ctypes.data) == want and step(k=py.ctypes.data - 504) == want and step(k=st.ctypes.data) == want
        assert step(tick_dev=kh.ctypes.data) == want and step(tick_dev=kh.ctypes.data + 504) == want
        if have_gpu:
            assert b"overlaps the input kh_t" in L.dlesm_last_error()

    assert step(tmask=None) == want
    if not have_gpu:
        assert b"no HIP device" in L.dlesm_last_error()
    # what dlesm_drifter_step_f64 refuses
    assert step(nsub=0) == want and step(nsub=1025) == want and step(h=float("nan")) == want and step(n=-1) == want
    assert step(x=None) == want and step(x=py.ctypes.data) == want
    if not walk:
        own()                                                        # the entry's own refusals stand where the entry looks
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
    if have_gpu:
        assert b"overlaps" in L.dlesm_last_error()
    if walk:
        own()
    handle = C.c_void_p(0x1234)
    k = kh.ctypes.data if walk else 1.0
    assert set_(None, 10.0, 1, k, 7, 0, None, 8, 8, 2, 7, 2, 7, t.ctypes.data, *fields, None) == want
    if not have_gpu:
        assert set_(handle, 10.0, 1, k, 7, 0, None, 8, 8, 2, 7, 2, 7, t.ctypes.data, *fields, None) == _cabi.ENODEV
    assert (px == 3.5).all() and (py == 4.5).all() and (st == 0).all() and (a == 1.0).all() and (t == 1).all()
    assert (tk == 5).all() and (ids == np.arange(8)).all() and (kh == 2.0).all()
