"""CPU tests of the boundary of the coupled distributed step and the int halo exchange: the header,
the library's exports, the ctypes table, the Fortran interfaces and INTEGRATION.md agree on dlesm_nemolite_coupled_step_dm,
dlesm_halo_exchange_i32 and the scheme enum, whose values are 0, 1, 2; the coupled entry's argument list is
dlesm_nemolite_step_wet_dm's with the scheme after the wet plan and the tracer arguments before the stream; a null plan is
refused without a device."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

from dl_esm_inf_amd import _cabi

L = _cabi.lib()
ENTRIES = ("dlesm_nemolite_coupled_step_dm", "dlesm_halo_exchange_i32")
ENUM = (("DLESM_TRACER_UPWIND", 0), ("DLESM_TRACER_MUSCL", 1), ("DLESM_TRACER_HANCOCK", 2))


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def _header():
    return re.sub(r"/\*.*?\*/", "", _read("include", "dlesm_hip.h"), flags=re.S)


def _decl(txt, name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, txt)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_exports_ctypes_and_documents_agree():
    txt = _header()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _cabi.LIB_PATH], text=True)
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    doc = _read("INTEGRATION.md")
    fortran = _read("dl_esm_inf_amd", "fortran", "dlesm_hip_mod.f90")
    for name in ENTRIES:
        args = _decl(txt, name)
        assert name in exported and name in _cabi.PROTOTYPES, name
        res, ctypes_args = _cabi.PROTOTYPES[name]
        assert res is C.c_int and len(ctypes_args) == len(args), name
        assert name in doc, name
        assert 'bind(C, name="%s")' % name in fortran, name
    # the coupled entry: dlesm_nemolite_step_wet_dm's arguments, the scheme after the wet plan, the tracers before the stream
    wet = _decl(txt, "dlesm_nemolite_step_wet_dm")
    tracer = _decl(txt, "dlesm_tracer_step_f64")
    assert _decl(txt, ENTRIES[0]) == wet[:2] + ["int scheme"] + wet[2:-1] + tracer[-4:]
    w = list(_cabi.PROTOTYPES["dlesm_nemolite_step_wet_dm"][1])
    t = list(_cabi.PROTOTYPES["dlesm_tracer_step_f64"][1])
    assert list(_cabi.PROTOTYPES[ENTRIES[0]][1]) == w[:2] + [C.c_int] + w[2:-1] + t[-4:]
    assert _decl(txt, ENTRIES[1]) == ["dlesm_halo_plan *plan", "int *field", "void *stream"]


def test_the_scheme_enum_is_0_1_2_everywhere():
    txt = _header()
    fortran = _read("dl_esm_inf_amd", "fortran", "dlesm_hip_mod.f90")
    doc = _read("INTEGRATION.md")
    for name, value in ENUM:
        m = re.search(r"\b%s\s*=\s*(\d+)" % name, txt)
        assert m and int(m.group(1)) == value, name
        m = re.search(r"\b%s\s*=\s*(\d+)_c_int" % name, fortran)
        assert m and int(m.group(1)) == value, name
        assert name in doc, name
    assert (_cabi.TRACER_UPWIND, _cabi.TRACER_MUSCL, _cabi.TRACER_HANCOCK) == (0, 1, 2)
    from dl_esm_inf_amd import psy
    assert psy.TRACER_SCHEMES == {"upwind": 0, "muscl": 1, "hancock": 2}


def test_wrappers_and_documents_exist():
    from dl_esm_inf_amd import grid_mod, psy
    assert callable(psy.invoke_nemolite_coupled_step_dm) and callable(grid_mod.exchange_mask_halos)
    psy_f = _read("dl_esm_inf_amd", "fortran", "dlesm_psy_mod.f90")
    grid_f = _read("dl_esm_inf_amd", "fortran", "dlesm_grid_mod.f90")
    assert "subroutine invoke_nemolite_coupled_step_dm(" in psy_f
    assert re.search(r"public ::[^\n]*\binvoke_nemolite_coupled_step_dm\b", psy_f)
    assert "subroutine exchange_mask_halos(" in grid_f and re.search(r"public [^\n]*\bexchange_mask_halos\b", grid_f)
    doc = _read("INTEGRATION.md")
    for name in ("invoke_nemolite_coupled_step_dm", "exchange_mask_halos"):
        assert name in doc, name
    design = _read("DESIGN.md")
    assert "### 6.13" in design and ENTRIES[0] in design and ENTRIES[1] in design
    assert "section 6.13" in _read("include", "dlesm_hip.h")


def test_null_pointers_are_refused_without_a_device():
    assert L.dlesm_nemolite_coupled_step_dm(None, None, 0, *[None] * 2, None, 8, 8, *[None] * 3, None, 0.0, *[None] * 13, None,
                                            None, 0, None) == _cabi.EINVAL
    assert b"dlesm_nemolite_coupled_step_dm: null plan" in L.dlesm_last_error()
    assert L.dlesm_halo_exchange_i32(None, None, None) == _cabi.EINVAL
    assert b"dlesm_halo_exchange_i32: null pointer" in L.dlesm_last_error()
