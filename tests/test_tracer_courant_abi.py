"""CPU tests of the boundary of the tracer schemes' Courant check: the record dlesm_tracer_courant is
64 bytes with the same members at the same offsets in the header, the ctypes table and the Fortran type; both entries are
exported from the product and from the lab build and stand in the ctypes table, INTEGRATION.md and dlesm_hip_mod with one
argument list; the HOOK key tracer_courant_kernel is classified; the Python names are public; without a GPU the entries fail
loudly and write nothing."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

import dl_esm_inf_amd as D
from dl_esm_inf_amd import _cabi

L = _cabi.lib()
ENTRIES = ("dlesm_tracer_courant_async_f64", "dlesm_tracer_courant_f64")
MEMBERS = [("face_max", "double"), ("outflow_max", "double"), ("face_index", "int64_t"), ("outflow_index", "int64_t"),
           ("face_over", "int64_t"), ("outflow_over", "int64_t"), ("invalid", "int64_t"), ("wet", "int64_t")]
ARRAYS = ["tmask", "area_t", "un", "vn", "hu", "hv", "ht", "sshn_t", "sshn_u", "sshn_v"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dlesm_hip.h")).read(), flags=re.S)


def _decl(txt, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_the_record_is_64_bytes_with_one_layout():
    m = re.search(r"typedef\s+struct\s+dlesm_tracer_courant\s*\{(.*?)\}\s*dlesm_tracer_courant\s*;", _header(), flags=re.S)
    assert m
    header = [(name, " ".join(typ.split())) for typ, name in re.findall(r"([\w ]+?)\s+(\w+)\s*;", m.group(1))]
    assert header == MEMBERS                                  # eight 8-byte members in this order: offsets 0, 8, .. 56
    T = _cabi.TracerCourant
    assert C.sizeof(T) == 64
    want = {"double": C.c_double, "int64_t": C.c_int64}
    assert [(n, t) for n, t in T._fields_] == [(n, want[t]) for n, t in MEMBERS]
    assert [getattr(T, n).offset for n, _ in MEMBERS] == list(range(0, 64, 8))
    fortran = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_hip_mod.f90")).read()
    m = re.search(r"type, bind\(C\) :: tracer_courant_type\n(.*?)end type tracer_courant_type", fortran, flags=re.S)
    assert m
    got = []
    for kind, names in re.findall(r"^\s*(real\(c_double\)|integer\(c_int64_t\)) :: (.*)$", m.group(1), flags=re.M):
        got += [(n.strip(), "double" if kind.startswith("real") else "int64_t") for n in names.split(",")]
    assert got == MEMBERS
    # the same through a C compiler, where there is one
    import shutil
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc:
        src = ('#include <stddef.h>\n#include <stdio.h>\n#include "dlesm_hip.h"\nint main(void){printf("%zu", '
               'sizeof(dlesm_tracer_courant));' +
               "".join('printf(" %%zu", offsetof(dlesm_tracer_courant, %s));' % n for n, _ in MEMBERS) + "return 0;}\n")
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            open(os.path.join(tmp, "t.c"), "w").write(src)
            subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "t.c"), "-o", os.path.join(tmp, "t")])
            out = subprocess.check_output([os.path.join(tmp, "t")], text=True).split()
        assert [int(x) for x in out] == [64] + list(range(0, 64, 8))


def test_header_exports_ctypes_and_documents_agree():
    txt = _header()
    libs = [_cabi.LIB_PATH, os.path.join(os.path.dirname(_cabi.LIB_PATH), "libdlesm_hip_lab.so")]
    for lib in libs:                                          # the product and the lab build
        out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        for name in ENTRIES:
            assert name in exported, (lib, name)
    step = _decl(txt, "dlesm_tracer_step_f64")
    for name in ENTRIES:
        args = _decl(txt, name)
        assert len(args) == 21
        assert args[:17] == [a for a in step[:18] if not a.endswith("ssha")]          # without ssha and the tracers
        assert [a.split("*")[-1].strip() for a in args[7:17]] == ARRAYS
        assert args[17:19] == ["double face_limit", "double outflow_limit"] and args[20] == "void *stream"
        res, ctypes_args = _cabi.PROTOTYPES[name]
        assert res is C.c_int and len(ctypes_args) == 21
        assert list(ctypes_args[:19]) == [C.c_double] + [C.c_int] * 6 + [C.c_void_p] * 10 + [C.c_double] * 2
        assert ctypes_args[20] is C.c_void_p
    assert _decl(txt, ENTRIES[0])[19] == "dlesm_tracer_courant *result_dev"
    assert _decl(txt, ENTRIES[1])[19] == "dlesm_tracer_courant *result_host"
    assert _cabi.PROTOTYPES[ENTRIES[0]][1][19] is C.c_void_p
    assert _cabi.PROTOTYPES[ENTRIES[1]][1][19] is C.POINTER(_cabi.TracerCourant)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES + ("dlesm_tracer_courant", "tracer_courant_kernel", "tracer_courant_type", "psy.tracer_courant",
                           "psy.tracer_courant_check"):
        assert name in doc, name
    assert "section 6.14" in open(os.path.join(ROOT, "include", "dlesm_hip.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 6.14" in design and "dlesm_tracer_courant_async_f64" in design
    fortran = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_hip_mod.f90")).read()
    for name in ENTRIES:
        m = re.search(r"function %s\((.*?)\)\s*bind\(C, name=\"%s\"\)" % (name, name), fortran, flags=re.S)
        assert m, name
        fargs = [a.strip() for a in m.group(1).replace("&", " ").split(",")]
        assert fargs == [a.split()[-1].lstrip("*") for a in _decl(txt, name)], name
    psy_f = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_psy_mod.f90")).read()
    assert "subroutine tracer_courant(" in psy_f and re.search(r"public ::[^\n]*\btracer_courant\b", psy_f)
    assert re.search(r"public ::[^\n]*\btracer_courant_type\b", psy_f)
    assert _cabi.lib().dlesm_version() == 310


def test_the_hook_key_is_classified():
    assert L.dlesm_tuning_class(b"tracer_courant_kernel") == L.dlesm_tuning_class(b"tracer_kernel") == 1
    settings = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    settings = settings[settings.index("## Settings"):]
    settings = settings[:settings.index("\n## ", 5)] if "\n## " in settings[5:] else settings
    assert "`tracer_courant_kernel`" not in settings                # a HOOK key is no user setting


def test_python_names_are_public():
    from dl_esm_inf_amd import psy
    assert D.TracerCourant is _cabi.TracerCourant
    assert callable(psy.tracer_courant) and callable(psy.tracer_courant_check)
    assert psy.TracerCourantResult._fields == ("face_max", "outflow_max", "face_at", "outflow_at", "face_over",
                                               "outflow_over", "invalid", "wet", "rdt_limit")
    r = _cabi.TracerCourant(0.25, 0.5, 3, 4, 5, 6, 7, 8)
    assert r.as8() == (0.25, 0.5, 3, 4, 5, 6, 7, 8) and "face_max=0.25" in repr(r) and "wet=8" in repr(r)


def test_without_a_gpu_the_entries_fail_loudly_and_write_nothing():
    """DLESM_ENODEV without a device; with one, host arrays of a valid shape pass every check that needs no device and the
    null pointer is refused"""
    a = np.ones((8, 8))
    t = np.ones((8, 8), dtype=np.int32)
    rec = _cabi.TracerCourant(1.0, 2.0, 3, 4, 5, 6, 7, 8)
    args = (20.0, 8, 8, 2, 7, 2, 7, None, *[a.ctypes.data] * 9, 0.5, 1.0)
    have_gpu = L.dlesm_device_count() > 0
    want = _cabi.EINVAL if have_gpu else _cabi.ENODEV
    assert L.dlesm_tracer_courant_f64(*args, C.byref(rec), None) == want
    if not have_gpu:
        assert b"no HIP device" in L.dlesm_last_error()
    assert L.dlesm_tracer_courant_async_f64(*args, C.byref(rec), None) == want
    assert L.dlesm_tracer_courant_async_f64(*args, None, None) == _cabi.EINVAL
    assert L.dlesm_tracer_courant_f64(*args, None, None) == _cabi.EINVAL
    assert rec.as8() == (1.0, 2.0, 3, 4, 5, 6, 7, 8) and (a == 1.0).all() and (t == 1).all()
