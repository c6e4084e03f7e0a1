"""CPU test: the C ABI of the land-skipping NEMOLite2D-class step -- the wet plan's three entries,
dlesm_nemolite_step_wet_f64 and dlesm_nemolite_step_wet_dm -- is the same in the header, both builds of the library, the
ctypes table, the Fortran bindings and INTEGRATION.md; the step entries take the plan, then every argument of the entries
they extend."""
import os
import re
import subprocess

from conftest import ROOT

from dl_esm_inf_amd import _cabi

NEW = ("dlesm_wet_plan_create", "dlesm_wet_plan_destroy", "dlesm_wet_plan_counts", "dlesm_nemolite_step_wet_f64",
       "dlesm_nemolite_step_wet_dm")


def _declared_arity(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dlesm_hip.h")).read(), flags=re.S)
    m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr)
    assert m, name
    return len(m.group(1).split(","))


def test_entries_are_exported_by_both_builds():
    for path in (_cabi.LIB_PATH, _cabi.LAB_BUILD_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(NEW) <= exported, path


def test_prototypes_have_the_headers_arity():
    P = _cabi.PROTOTYPES
    for name in NEW:
        assert len(P[name][1]) == _declared_arity(name), name
    assert len(P["dlesm_wet_plan_create"][1]) == 5 and len(P["dlesm_wet_plan_counts"][1]) == 3
    # the plan first (after the halo plan in the distributed entry), then the arguments of the entry it extends
    assert P["dlesm_nemolite_step_wet_f64"][1] == [_cabi.C.c_void_p] + P["dlesm_nemolite_step_f64"][1]
    dm = P["dlesm_nemolite_step_dm"][1]
    assert P["dlesm_nemolite_step_wet_dm"][1] == dm[:1] + [_cabi.C.c_void_p] + dm[1:]
    assert P["dlesm_wet_plan_counts"][1][1]._type_ is _cabi.C.c_longlong


def test_entries_are_bound_in_fortran_and_named_in_the_documents():
    f90 = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_hip_mod.f90")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert f'bind(C, name="{name}")' in f90, name
        assert name in doc, name
    psy = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_psy_mod.f90")).read()
    assert re.search(r"public ::.*\bwet_plan\b", psy)
    assert len(re.findall(r"logical, intent\(in\), optional :: skip_land", psy)) == 2
    assert "psy.wet_plan" in doc and "skip_land" in doc


def test_plan_host_side_needs_no_device():
    """an empty box gives a plan of no tiles, and the plan's own refusals come before any device call"""
    import ctypes as C

    import numpy as np
    L = _cabi.lib()
    tm = np.ones((12, 40), dtype=np.int32)
    R = lambda *b: C.byref(_cabi.Region(0, 0, *b))  # noqa: E731
    h = C.c_void_p()
    assert L.dlesm_wet_plan_create(tm.ctypes.data, 40, 12, R(5, 4, 2, 2), C.byref(h)) == 0 and h.value
    t, a = C.c_longlong(-1), C.c_longlong(-1)
    assert L.dlesm_wet_plan_counts(h, C.byref(t), C.byref(a)) == 0 and (t.value, a.value) == (0, 0)
    assert L.dlesm_wet_plan_destroy(h) == 0 and L.dlesm_wet_plan_destroy(None) == 0
    h = C.c_void_p()
    for args in ((None, 40, 12, R(2, 39, 2, 11)), (tm.ctypes.data, 40, 12, None), (tm.ctypes.data, 0, 12, R(2, 39, 2, 11)),
                 (tm.ctypes.data, 40, 12, R(1, 39, 2, 11)), (tm.ctypes.data, 40, 12, R(2, 40, 2, 11)),
                 (tm.ctypes.data, 40, 12, R(2, 39, 2, 12))):
        assert L.dlesm_wet_plan_create(*args, C.byref(h)) == _cabi.EINVAL and not h.value, args
    assert L.dlesm_wet_plan_create(tm.ctypes.data, 40, 12, R(2, 39, 2, 11), None) == _cabi.EINVAL
    assert L.dlesm_wet_plan_counts(None, C.byref(t), C.byref(a)) == _cabi.EINVAL
