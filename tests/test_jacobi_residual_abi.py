"""CPU test: the C ABI of the Jacobi step with its residual (dlesm_stencil5_resid_f64, dlesm_global_max_f64) is the same in the
header, both builds of the library, the ctypes table and the Fortran bindings -- the norm codes included."""
import os
import re
import subprocess

from conftest import ROOT

from dl_esm_inf_amd import _cabi

NEW = ("dlesm_stencil5_resid_f64", "dlesm_global_max_f64")


def test_norm_codes_agree():
    hdr = open(os.path.join(ROOT, "include", "dlesm_hip.h")).read()
    m = re.search(r"enum\s*\{\s*DLESM_NORM_MAX\s*=\s*(\d+)\s*,\s*DLESM_NORM_SUMSQ\s*=\s*(\d+)\s*\}", hdr)
    assert m, "include/dlesm_hip.h declares the norm codes"
    assert (int(m.group(1)), int(m.group(2))) == (_cabi.NORM_MAX, _cabi.NORM_SUMSQ) == (0, 1)
    f90 = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_hip_mod.f90")).read()
    assert re.search(r"DLESM_NORM_MAX\s*=\s*0_c_int,\s*DLESM_NORM_SUMSQ\s*=\s*1_c_int", f90)


def test_entries_are_exported_and_bound():
    for path in (_cabi.LIB_PATH, _cabi.LAB_BUILD_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(NEW) <= exported, path
    assert _cabi.PROTOTYPES["dlesm_stencil5_resid_f64"][1][8] is _cabi.C.c_int          # norm: by value, after the box
    assert len(_cabi.PROTOTYPES["dlesm_stencil5_resid_f64"][1]) == 11
    f90 = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_hip_mod.f90")).read()
    for name in NEW:
        assert f'bind(C, name="{name}")' in f90, name
    psy = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_psy_mod.f90")).read()
    assert re.search(r"public ::.*\binvoke_jacobi5_residual\b", psy)
