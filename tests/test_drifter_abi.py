"""CPU tests of the boundary of the drifters: the seven entries are exported from the product and
from the lab build and stand in the header, the ctypes table, INTEGRATION.md and dlesm_hip_mod with one argument list each;
the DLESM_DRIFTER_* numbers are the same in the header, the ctypes module, the Fortran module and the restatement; the Python
and Fortran names are public; dlesm_version() is unchanged; without a GPU the entries fail loudly and write nothing."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

import dl_esm_inf_amd as D
from dl_esm_inf_amd import _cabi

import drifter_numpy as DN

L = _cabi.lib()
_i, _d, _vp, _ll = C.c_int, C.c_double, C.c_void_p, C.c_longlong
ENTRIES = {
    "dlesm_drifter_step_f64": (
        ["double h", "int nsub", "int ld", "int ny", "int xstart", "int xstop", "int ystart", "int ystop", "const int *tmask",
         "const double *dx_t", "const double *dy_t", "const double *un", "const double *vn", "long long n", "double *px",
         "double *py", "int *status", "void *stream"],
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
}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dlesm_hip.h")).read(), flags=re.S)


def _names(args):
    return [a.split()[-1].lstrip("*") for a in args]


def test_header_exports_ctypes_and_documents_agree():
    txt = _header()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    fortran = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_hip_mod.f90")).read()
    exported = []
    for lib in [_cabi.LIB_PATH, os.path.join(os.path.dirname(_cabi.LIB_PATH), "libdlesm_hip_lab.so")]:
        out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
        exported.append({l.split()[-1] for l in out.splitlines() if " T " in l})
    for entry, (args, ctypes_args) in ENTRIES.items():
        assert entry in exported[0] and entry in exported[1], entry
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % entry, txt)
        assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == args, entry
        res, got = _cabi.PROTOTYPES[entry]
        assert res is C.c_int and list(got) == ctypes_args, entry
        m = re.search(r"`%s\(([^)]*)\)`" % entry, doc)
        assert m and [a.strip() for a in m.group(1).replace("\n", " ").split(",")] == _names(args), entry
        m = re.search(r"function %s\((.*?)\)\s*bind\(C, name=\"%s\"\)" % (entry, entry), fortran, flags=re.S)
        assert m and [a.strip() for a in m.group(1).replace("&", " ").split(",")] == _names(args), entry
    assert {e for e in exported[0] if "drifter" in e} == set(ENTRIES)
    assert re.search(r"typedef struct dlesm_drifters dlesm_drifters;", txt)
    for name in ("psy.drifter_step", "psy.drifter_sample", "call drifter_step(", "call drifters_create(", "call drifters_get(",
                 "call drifters_free(", "drifters_type", "DLESM_DRIFTER_ACTIVE", "DLESM_DRIFTER_LEFT", "DLESM_DRIFTER_OPEN",
                 "DLESM_DRIFTER_GROUNDED", "DLESM_DRIFTER_MAX_SUB", "DLESM_DRIFTER_MAX_FIELDS"):
        assert name in doc, name
    raw = open(os.path.join(ROOT, "include", "dlesm_hip.h")).read()
    assert raw.count("section 6.17") >= 2                            # the entries' comment and the owner's
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 6.17 Drifters (frozen here)" in design and all(e in design for e in ENTRIES)
    assert L.dlesm_version() == 310


def test_the_status_numbers_agree():
    h = _header()
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


def test_the_wrappers_are_public():
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


def test_without_a_gpu_the_entries_fail_loudly_and_write_nothing():
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
