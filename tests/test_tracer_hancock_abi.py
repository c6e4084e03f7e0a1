"""CPU tests of the boundary of the time-centred limited tracer entries: the header, the library's
exports, the ctypes table and INTEGRATION.md agree on dlesm_tracer_step_hancock_f64 / dlesm_tracer_step_hancock_dm, whose
argument lists are those of the upwind entries; the HOOK key tracer_hancock_kernel is classified; without a GPU the entries
fail loudly, every DLESM_EINVAL of section 6.10 that can be told without a device comes first or second as it does for the
upwind entry, a null plan is refused, and nothing is written."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

from dl_esm_inf_amd import _cabi

L = _cabi.lib()
PAIRS = (("dlesm_tracer_step_hancock_f64", "dlesm_tracer_step_f64"), ("dlesm_tracer_step_hancock_dm", "dlesm_tracer_step_dm"))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dlesm_hip.h")).read(), flags=re.S)


def _decl(txt, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_exports_ctypes_and_documents_agree():
    txt = _header()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _cabi.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name, upwind in PAIRS:
        args = _decl(txt, name)
        assert args == _decl(txt, upwind), name                   # dlesm_tracer_step_f64's argument list, word for word
        assert name in exported and name in _cabi.PROTOTYPES
        res, ctypes_args = _cabi.PROTOTYPES[name]
        assert res is C.c_int and len(ctypes_args) == len(args) == (22 if name.endswith("f64") else 23)
        assert list(ctypes_args) == list(_cabi.PROTOTYPES[upwind][1])
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in [p[0] for p in PAIRS] + ["tracer_hancock_kernel", "invoke_tracer_step_hancock", "invoke_tracer_step_hancock_dm"]:
        assert name in doc, name
    raw = open(os.path.join(ROOT, "include", "dlesm_hip.h")).read()
    assert "section 6.12" in raw
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 6.12" in design and "dlesm_tracer_step_hancock_f64" in design
    fortran = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_hip_mod.f90")).read()
    for name, _ in PAIRS:
        assert 'bind(C, name="%s")' % name in fortran
    psy_f = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_psy_mod.f90")).read()
    for name in ("invoke_tracer_step_hancock", "invoke_tracer_step_hancock_dm"):
        assert "subroutine %s(" % name in psy_f and re.search(r"public ::[^\n]*\b%s\b" % name, psy_f), name


def test_python_wrappers_exist():
    from dl_esm_inf_amd import psy
    assert callable(psy.invoke_tracer_step_hancock) and callable(psy.invoke_tracer_step_hancock_dm)


def test_the_hook_key_is_classified():
    assert L.dlesm_tuning_class(b"tracer_hancock_kernel") == L.dlesm_tuning_class(b"tracer_kernel") == 1
    settings = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    settings = settings[settings.index("## Settings"):]
    settings = settings[:settings.index("\n## ", 5)] if "\n## " in settings[5:] else settings
    assert "`tracer_hancock_kernel`" not in settings                # a HOOK key is no user setting


def _args(out, a=None, t=None, box=(2, 7, 2, 7), k=1, pin=None, pout=None):
    a = np.ones((8, 8)) if a is None else a
    t = np.ones((8, 8), dtype=np.int32) if t is None else t
    pin = (C.c_void_p * 1)(a.ctypes.data) if pin is None else pin
    pout = (C.c_void_p * 1)(out.ctypes.data) if pout is None else pout
    keep = (a, t, pin, pout)
    return keep, (20.0, 8, 8, *box, t.ctypes.data, *[a.ctypes.data] * 10, pin, pout, k, None)


def test_no_gpu_fails_loudly_not_silently():
    """without a device dlesm_tracer_step_hancock_f64 is DLESM_ENODEV and writes nothing.  dlesm_tracer_step_hancock_dm needs a
    halo plan, and a plan cannot be made without a device; the null plan that is left is refused"""
    if L.dlesm_device_count() > 0:
        pytest.skip("a GPU is present")
    out = np.full((8, 8), -7.0)
    keep, args = _args(out)
    assert L.dlesm_tracer_step_hancock_f64(*args) == _cabi.ENODEV
    assert b"no HIP device" in L.dlesm_last_error()
    tables = _cabi.CommTables()
    plan = C.c_void_p()
    assert L.dlesm_halo_plan_create(C.byref(tables), 8, 8, C.byref(plan)) == _cabi.ENODEV
    assert L.dlesm_tracer_step_hancock_dm(None, *args) == _cabi.EINVAL
    assert b"dlesm_tracer_step_hancock_dm: null plan" in L.dlesm_last_error()
    assert (out == -7.0).all()


def test_refusals_match_the_upwind_entrys():
    """every refusal of section 6.10 -- the tracer count, null pointers, a box without its ring, an output over an input, a
    c_in or another output -- gets from dlesm_tracer_step_hancock_f64 the code dlesm_tracer_step_f64 gives for the same
    arguments (DLESM_EINVAL on a machine with a device, where the check runs; DLESM_ENODEV without one, where the device is
    asked for first), and nothing is written either way"""
    out = np.full((8, 8), -7.0)
    a = np.ones((8, 8))
    two_in = (C.c_void_p * 2)(a.ctypes.data, a.ctypes.data)
    cases = {
        "k=0": dict(k=0), "k=9": dict(k=9), "k=-1": dict(k=-1),
        "no west ring": dict(box=(1, 7, 2, 7)), "no east ring": dict(box=(2, 8, 2, 7)),
        "no south ring": dict(box=(2, 7, 1, 7)), "no north ring": dict(box=(2, 7, 2, 8)),
        "out is in": dict(a=a, pout=(C.c_void_p * 1)(a.ctypes.data)),
        "out twice": dict(k=2, pin=two_in, pout=(C.c_void_p * 2)(out.ctypes.data, out.ctypes.data)),
        "null c_out[1]": dict(k=2, pin=two_in, pout=(C.c_void_p * 2)(out.ctypes.data, None)),
        "null c_in[0]": dict(pin=(C.c_void_p * 1)(None)),
    }
    have_gpu = L.dlesm_device_count() > 0
    for what, kw in cases.items():
        keep, args = _args(out, **kw)
        rc_up = L.dlesm_tracer_step_f64(*args)
        rc = L.dlesm_tracer_step_hancock_f64(*args)
        assert rc == rc_up == (_cabi.EINVAL if have_gpu else _cabi.ENODEV), (what, rc, rc_up)
        assert b"dlesm_tracer_step_hancock_f64" in L.dlesm_last_error() or not have_gpu, what
        assert L.dlesm_tracer_step_hancock_dm(None, *args) == _cabi.EINVAL, what
    assert (out == -7.0).all() and (a == 1.0).all()
