"""CPU tests of the boundary of the flow step's stability check: the record dlesm_flow_courant is 128
bytes with the same members at the same offsets in the header, the ctypes table and the Fortran type; both entries are
exported from the product and from the lab build and stand in the ctypes table, INTEGRATION.md and dlesm_hip_mod with one
argument list; the HOOK key flow_courant_kernel is classified; the Python names are public; dlesm_version() is unchanged;
without a GPU the entries fail loudly and write nothing."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

from conftest import ROOT

import dl_esm_inf_amd as D
from dl_esm_inf_amd import _cabi

L = _cabi.lib()
ENTRIES = ("dlesm_flow_courant_async_f64", "dlesm_flow_courant_f64")
DOUBLES = ["gravity_max", "advective_max", "viscous_max", "depth_min"]
INTS = ["gravity_index", "advective_index", "viscous_index", "depth_index", "gravity_over", "advective_over", "viscous_over",
        "shallow", "invalid", "wet"]
MEMBERS = [(n, "double") for n in DOUBLES] + [(n, "int64_t") for n in INTS] + [("reserved[2]", "int64_t")]
OFFSETS = list(range(0, 120, 8))                              # the fourteen 8-byte members, then reserved[2] at 112
ARRAYS = ["tmask", "dx_t", "dy_t", "un", "vn", "ht", "sshn_t"]
SCALARS = ["double rdt", "double g", "double visc", "int ld", "int ny", "int xstart", "int xstop", "int ystart", "int ystop"]
LIMITS = ["double gravity_limit", "double advective_limit", "double viscous_limit", "double depth_limit"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dlesm_hip.h")).read(), flags=re.S)


def _decl(txt, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_the_record_is_128_bytes_with_one_layout():
    m = re.search(r"typedef\s+struct\s+dlesm_flow_courant\s*\{(.*?)\}\s*dlesm_flow_courant\s*;", _header(), flags=re.S)
    assert m
    header = []
    for typ, names in re.findall(r"(double|int64_t)\s+([^;]+);", m.group(1)):
        header += [(n.strip(), typ) for n in names.split(",")]
    assert header == MEMBERS
    T = _cabi.FlowCourant
    assert C.sizeof(T) == 128
    assert [(n, t) for n, t in T._fields_] == ([(n, C.c_double) for n in DOUBLES] + [(n, C.c_int64) for n in INTS] +
                                               [("reserved", C.c_int64 * 2)])
    assert [getattr(T, n).offset for n, _ in T._fields_] == OFFSETS
    fortran = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_hip_mod.f90")).read()
    m = re.search(r"type, bind\(C\) :: flow_courant_type\n(.*?)end type flow_courant_type", fortran, flags=re.S)
    assert m
    got = []
    for kind, names in re.findall(r"^\s*(real\(c_double\)|integer\(c_int64_t\)) :: (.*)$", m.group(1), flags=re.M):
        got += [(n.strip().replace("(2)", "[2]"), "double" if kind.startswith("real") else "int64_t")
                for n in names.split(",")]
    assert got == MEMBERS
    cc = shutil.which("cc") or shutil.which("gcc")            # the same through a C compiler, where there is one
    if cc:
        names = DOUBLES + INTS + ["reserved"]
        src = ('#include <stddef.h>\n#include <stdio.h>\n#include "dlesm_hip.h"\nint main(void){printf("%zu", '
               'sizeof(dlesm_flow_courant));' +
               "".join('printf(" %%zu", offsetof(dlesm_flow_courant, %s));' % n for n in names) + "return 0;}\n")
        with tempfile.TemporaryDirectory() as tmp:
            open(os.path.join(tmp, "t.c"), "w").write(src)
            subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "t.c"), "-o", os.path.join(tmp, "t")])
            out = subprocess.check_output([os.path.join(tmp, "t")], text=True).split()
        assert [int(x) for x in out] == [128] + OFFSETS


def test_header_exports_ctypes_and_documents_agree():
    txt = _header()
    libs = [_cabi.LIB_PATH, os.path.join(os.path.dirname(_cabi.LIB_PATH), "libdlesm_hip_lab.so")]
    for lib in libs:                                          # the product and the lab build
        out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        for name in ENTRIES:
            assert name in exported, (lib, name)
    for name in ENTRIES:
        args = _decl(txt, name)
        assert len(args) == 22
        assert args[:9] == SCALARS
        assert args[9] == "const int *tmask" and args[10:16] == ["const double *" + a for a in ARRAYS[1:]]
        assert args[16:20] == LIMITS and args[21] == "void *stream"
        res, ctypes_args = _cabi.PROTOTYPES[name]
        assert res is C.c_int and len(ctypes_args) == 22
        assert list(ctypes_args[:20]) == [C.c_double] * 3 + [C.c_int] * 6 + [C.c_void_p] * 7 + [C.c_double] * 4
        assert ctypes_args[21] is C.c_void_p
    assert _decl(txt, ENTRIES[0])[20] == "dlesm_flow_courant *result_dev"
    assert _decl(txt, ENTRIES[1])[20] == "dlesm_flow_courant *result_host"
    assert _cabi.PROTOTYPES[ENTRIES[0]][1][20] is C.c_void_p
    assert _cabi.PROTOTYPES[ENTRIES[1]][1][20] is C.POINTER(_cabi.FlowCourant)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES + ("dlesm_flow_courant", "flow_courant_kernel", "flow_courant_type", "psy.flow_courant",
                           "psy.flow_courant_check", "psy.step_rdt_limit"):
        assert name in doc, name
    assert "section 6.15" in open(os.path.join(ROOT, "include", "dlesm_hip.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 6.15" in design and "dlesm_flow_courant_async_f64" in design
    fortran = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_hip_mod.f90")).read()
    for name in ENTRIES:
        m = re.search(r"function %s\((.*?)\)\s*bind\(C, name=\"%s\"\)" % (name, name), fortran, flags=re.S)
        assert m, name
        fargs = [a.strip() for a in m.group(1).replace("&", " ").split(",")]
        assert fargs == [a.split()[-1].lstrip("*") for a in _decl(txt, name)], name
    psy_f = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_psy_mod.f90")).read()
    assert "subroutine flow_courant(" in psy_f and re.search(r"public ::[^\n]*\bflow_courant\b", psy_f)
    assert re.search(r"public ::[^\n]*\bflow_courant_type\b", psy_f)
    assert _cabi.lib().dlesm_version() == 310


def test_the_hook_key_is_classified():
    assert L.dlesm_tuning_class(b"flow_courant_kernel") == L.dlesm_tuning_class(b"tracer_courant_kernel") == 1
    settings = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    settings = settings[settings.index("## Settings"):]
    settings = settings[:settings.index("\n## ", 5)] if "\n## " in settings[5:] else settings
    assert "`flow_courant_kernel`" not in settings                  # a HOOK key is no user setting


def test_python_names_are_public():
    from dl_esm_inf_amd import psy
    assert D.FlowCourant is _cabi.FlowCourant
    assert callable(psy.flow_courant) and callable(psy.flow_courant_check) and callable(psy.step_rdt_limit)
    assert psy.FlowCourantResult._fields == (
        "gravity_max", "advective_max", "viscous_max", "depth_min", "gravity_at", "advective_at", "viscous_at", "depth_at",
        "gravity_over", "advective_over", "viscous_over", "shallow", "invalid", "wet", "rdt_limit")
    r = _cabi.FlowCourant(0.25, 0.5, 0.75, 1.5, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, (13, 14))
    assert r.as16() == (0.25, 0.5, 0.75, 1.5, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14)
    assert "gravity_max=0.25" in repr(r) and "wet=12" in repr(r)
    import inspect
    sig = inspect.signature(psy.flow_courant).parameters
    assert list(sig)[:5] == ["rdt", "un", "vn", "ht", "sshn_t"]
    assert [sig[k].default for k in ("gravity_limit", "advective_limit", "viscous_limit", "depth_limit")] == [1.0, 1.0, 0.25, 0.0]


def test_without_a_gpu_the_entries_fail_loudly_and_write_nothing():
    """DLESM_ENODEV without a device; with one, host arrays of a valid shape pass every check that needs no device and the
    null pointer is refused"""
    a = np.ones((8, 8))
    t = np.ones((8, 8), dtype=np.int32)
    before = (1.0, 2.0, 3.0, 4.0, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14)
    rec = _cabi.FlowCourant(*before[:14], before[14:])
    args = (20.0, 9.8, 1.0, 8, 8, 2, 7, 2, 7, None, *[a.ctypes.data] * 6, 1.0, 1.0, 0.25, 0.0)
    have_gpu = L.dlesm_device_count() > 0
    want = _cabi.EINVAL if have_gpu else _cabi.ENODEV
    assert L.dlesm_flow_courant_f64(*args, C.byref(rec), None) == want
    if not have_gpu:
        assert b"no HIP device" in L.dlesm_last_error()
    assert L.dlesm_flow_courant_async_f64(*args, C.byref(rec), None) == want
    assert L.dlesm_flow_courant_async_f64(*args, None, None) == _cabi.EINVAL
    assert L.dlesm_flow_courant_f64(*args, None, None) == _cabi.EINVAL
    assert rec.as16() == before and (a == 1.0).all() and (t == 1).all()
