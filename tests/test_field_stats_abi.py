"""CPU test: the C ABI of the field statistics (dlesm_field_stats_async_f64, dlesm_field_stats_f64, dlesm_field_locate_f64) is
the same in the header, both builds of the library, the ctypes table and the Fortran bindings -- the record's layout and the
enum values included."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

from dl_esm_inf_amd import _cabi

NEW = ("dlesm_field_stats_async_f64", "dlesm_field_stats_f64", "dlesm_field_locate_f64")
MEMBERS = ("min", "max", "sum", "sumsq", "count", "nonfinite")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_record_layout_agrees():
    S = _cabi.FieldStats
    assert C.sizeof(S) == 48
    assert tuple(n for n, _ in S._fields_) == MEMBERS
    assert [getattr(S, n).offset for n in MEMBERS] == [0, 8, 16, 24, 32, 40]
    assert [t for _, t in S._fields_] == [C.c_double] * 4 + [C.c_int64] * 2
    hdr = re.sub(r"/\*.*?\*/", "", _read("include", "dlesm_hip.h"), flags=re.S)
    m = re.search(r"typedef struct dlesm_field_stats\s*\{(.*?)\}\s*dlesm_field_stats;", hdr, flags=re.S)
    assert m, "include/dlesm_hip.h declares dlesm_field_stats"
    decl = [(t, [n.strip() for n in names.split(",")]) for t, names in re.findall(r"(double|int64_t)\s+([^;]+);", m.group(1))]
    assert [n for _, names in decl for n in names] == list(MEMBERS)
    assert [t for t, names in decl for _ in names] == ["double"] * 4 + ["int64_t"] * 2
    f90 = _read("dl_esm_inf_amd", "fortran", "dlesm_hip_mod.f90")
    m = re.search(r"type, bind\(C\) :: field_stats_type(.*?)end type field_stats_type", f90, flags=re.S)
    assert m, "dlesm_hip_mod declares field_stats_type"
    assert re.search(r"real\(c_double\) :: min, max, sum, sumsq\s+integer\(c_int64_t\) :: count, nonfinite\s*$", m.group(1).rstrip() + "\n",
                     flags=re.S)


def test_enum_values_agree():
    hdr = _read("include", "dlesm_hip.h")
    f90 = _read("dl_esm_inf_amd", "fortran", "dlesm_hip_mod.f90")
    m = re.search(r"enum\s*\{\s*DLESM_LOCATE_NONFINITE\s*=\s*(\d+)\s*,\s*DLESM_LOCATE_EQUAL\s*=\s*(\d+)\s*\}", hdr)
    assert m, "include/dlesm_hip.h declares the locate codes"
    assert (int(m.group(1)), int(m.group(2))) == (_cabi.LOCATE_NONFINITE, _cabi.LOCATE_EQUAL) == (0, 1)
    assert re.search(r"DLESM_LOCATE_NONFINITE\s*=\s*0_c_int,\s*DLESM_LOCATE_EQUAL\s*=\s*1_c_int", f90)
    m = re.search(r"enum\s*\{\s*DLESM_STATS_MAX_FIELDS\s*=\s*(\d+)\s*\}", hdr)
    assert m and int(m.group(1)) == _cabi.STATS_MAX_FIELDS == 8
    assert re.search(r"DLESM_STATS_MAX_FIELDS\s*=\s*8_c_int", f90)


def test_entries_are_exported_and_bound():
    for path in (_cabi.LIB_PATH, _cabi.LAB_BUILD_PATH):
        out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
        exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
        assert set(NEW) <= exported, path
    for name in NEW[:2]:
        args = _cabi.PROTOTYPES[name][1]
        assert len(args) == 8 and args[3:6] == [C.c_int] * 3          # nfields, ld, ny by value, after the three arrays
    assert _cabi.PROTOTYPES["dlesm_field_stats_f64"][1][6] is C.POINTER(_cabi.FieldStats)
    args = _cabi.PROTOTYPES["dlesm_field_locate_f64"][1]
    assert len(args) == 12 and args[8] is C.c_int and args[9] is C.c_double and args[10] is C.POINTER(C.c_int64)
    f90 = _read("dl_esm_inf_amd", "fortran", "dlesm_hip_mod.f90")
    for name in NEW:
        assert f'bind(C, name="{name}")' in f90, name
    fld = _read("dl_esm_inf_amd", "fortran", "dlesm_field_mod.f90")
    assert re.search(r"public ::.*\bfield_stats\b", fld) and re.search(r"public ::.*\bfield_locate\b", fld)
    assert re.search(r"subroutine field_stats\(fld, stats, mask\)", fld)


def test_python_names_are_public():
    import dl_esm_inf_amd as D
    assert D.FieldStats is _cabi.FieldStats
    assert callable(D.field_stats) and callable(D.field_locate) and callable(D.psy.run_health)
    doc = _read("INTEGRATION.md")
    for name in NEW + ("dlesm_field_stats",):
        assert name in doc, name
