"""CPU tests of the boundary of the model's output fields: dlesm_flow_output_f64 is exported from the
product and from the lab build and stands in the header, the ctypes table, INTEGRATION.md and dlesm_hip_mod with one argument
list; the DLESM_OUT_* numbers are the same in the header, the ctypes module and the restatement; the HOOK key
flow_output_kernel is classified; the Python name is public; dlesm_version() is unchanged; without a GPU the entry fails
loudly and writes nothing."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

import dl_esm_inf_amd as D
from dl_esm_inf_amd import _cabi

import flow_output_numpy as ON

L = _cabi.lib()
ENTRY = "dlesm_flow_output_f64"
ARGS = ["int mode", "double weight", "int ld", "int ny", "int xstart", "int xstop", "int ystart", "int ystop",
        "const int *tmask", "const double *dx_v", "const double *dy_u", "const double *un", "const double *vn",
        "const double *ht", "const double *sshn_t", "double *const *out", "void *stream"]
NAMES = [a.split()[-1].lstrip("*") for a in ARGS]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dlesm_hip.h")).read(), flags=re.S)


def test_header_exports_ctypes_and_documents_agree():
    txt = _header()
    for lib in [_cabi.LIB_PATH, os.path.join(os.path.dirname(_cabi.LIB_PATH), "libdlesm_hip_lab.so")]:
        out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
        assert ENTRY in {l.split()[-1] for l in out.splitlines() if " T " in l}, lib
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % ENTRY, txt)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == ARGS
    assert "_dm" not in "".join(re.findall(r"dlesm_flow_output\w*", txt)).replace(ENTRY, "")     # no distributed twin
    res, args = _cabi.PROTOTYPES[ENTRY]
    assert res is C.c_int
    assert list(args) == [C.c_int, C.c_double] + [C.c_int] * 6 + [C.c_void_p] * 7 + [C.POINTER(C.c_void_p), C.c_void_p]
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"`%s\(([^)]*)\)`" % ENTRY, doc)
    assert m and [a.strip() for a in m.group(1).replace("\n", " ").split(",")] == NAMES
    for name in ("flow_output_kernel", "psy.flow_output", "call flow_output(", "DLESM_OUT_SET", "DLESM_OUT_ADD",
                 "DLESM_OUT_COUNT"):
        assert name in doc, name
    assert "section 6.16" in open(os.path.join(ROOT, "include", "dlesm_hip.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 6.16 The model's output fields (frozen here)" in design and ENTRY in design
    fortran = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_hip_mod.f90")).read()
    m = re.search(r"function %s\((.*?)\)\s*bind\(C, name=\"%s\"\)" % (ENTRY, ENTRY), fortran, flags=re.S)
    assert m and [a.strip() for a in m.group(1).replace("&", " ").split(",")] == NAMES
    psy_f = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_psy_mod.f90")).read()
    assert re.search(r"public ::[^\n]*\bflow_output\b", psy_f)
    m = re.search(r"subroutine flow_output\(([^)]*)\)", psy_f)
    assert m and [a.strip() for a in m.group(1).split(",")] == ["un", "vn", "ht", "sshn_t", "ssh", "ut", "vt", "speed", "ke",
                                                                 "vort", "weight"]
    assert L.dlesm_version() == 310


def test_the_output_numbers_agree():
    m = re.search(r"enum\s*\{\s*DLESM_OUT_SSH = 0,([^}]*)\}", _header())
    assert m and [a.strip() for a in m.group(1).split(",")] == ["DLESM_OUT_UT", "DLESM_OUT_VT", "DLESM_OUT_SPEED",
                                                                "DLESM_OUT_KE", "DLESM_OUT_VORT", "DLESM_OUT_COUNT"]
    assert re.search(r"enum\s*\{\s*DLESM_OUT_SET = 0,\s*DLESM_OUT_ADD = 1\s*\}", _header())
    ours = (_cabi.OUT_SSH, _cabi.OUT_UT, _cabi.OUT_VT, _cabi.OUT_SPEED, _cabi.OUT_KE, _cabi.OUT_VORT, _cabi.OUT_COUNT)
    assert ours == (ON.SSH, ON.UT, ON.VT, ON.SPEED, ON.KE, ON.VORT, ON.COUNT) == tuple(range(7))
    assert (_cabi.OUT_SET, _cabi.OUT_ADD) == (ON.SET, ON.ADD) == (0, 1)


def test_the_hook_key_is_classified():
    assert L.dlesm_tuning_class(b"flow_output_kernel") == L.dlesm_tuning_class(b"flow_courant_kernel") == 1
    settings = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    settings = settings[settings.index("## Settings"):]
    settings = settings[:settings.index("\n## ", 5)] if "\n## " in settings[5:] else settings
    assert "`flow_output_kernel`" not in settings                   # a HOOK key is no user setting


def test_the_python_name_is_public():
    from dl_esm_inf_amd import psy
    assert D.flow_output is psy.flow_output and callable(psy.flow_output)
    sig = inspect.signature(psy.flow_output).parameters
    assert list(sig)[:11] == ["un", "vn", "ht", "sshn_t", "ssh", "ut", "vt", "speed", "ke", "vort", "weight"]
    assert all(sig[k].default is None for k in list(sig)[4:11])
    assert tuple(list(sig)[4:10]) == ON.NAMES


def test_without_a_gpu_the_entry_fails_loudly_and_writes_nothing():
    """DLESM_ENODEV without a device; with one, host arrays of a valid shape pass every check that needs no device and the
    null pointers are refused"""
    a = np.ones((8, 8))
    t = np.ones((8, 8), dtype=np.int32)
    o = np.full((8, 8), -7.0)
    out = (C.c_void_p * 6)(*[o.ctypes.data] * 6)
    have_gpu = L.dlesm_device_count() > 0
    want = _cabi.EINVAL if have_gpu else _cabi.ENODEV
    args = (0, 0.0, 8, 8, 2, 7, 2, 7, None, *[a.ctypes.data] * 6)
    assert L.dlesm_flow_output_f64(*args, out, None) == want                     # (a null mask, where there is a device)
    if not have_gpu:
        assert b"no HIP device" in L.dlesm_last_error()
    args = (0, 0.0, 8, 8, 2, 7, 2, 7, t.ctypes.data, *[a.ctypes.data] * 6)
    assert L.dlesm_flow_output_f64(*args, None, None) == want
    assert L.dlesm_flow_output_f64(*args, (C.c_void_p * 6)(), None) == want
    assert L.dlesm_flow_output_f64(5, 0.0, *args[2:], out, None) == want
    assert (o == -7.0).all() and (a == 1.0).all() and (t == 1).all()
