"""CPU tests of the boundary of the particle order: the five entries are exported from the product and
from the lab build and stand in the header, the ctypes table, INTEGRATION.md and dlesm_hip_mod with one argument list each;
none of their names contains `drifter` (tests/test_particle_steps_abi.py pins that set); dlesm_version() is unchanged; the Python and
Fortran names are public; the scratch query is host arithmetic; without a GPU the entries fail loudly and write nothing, and
with one every refusal is DLESM_EINVAL with nothing written."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

import dl_esm_inf_amd as D
from dl_esm_inf_amd import _cabi

import particle_order_cases as PC

L = _cabi.lib()
_i, _vp, _ll = C.c_int, C.c_void_p, C.c_longlong
ENTRIES = {
    "dlesm_particle_order_scratch": (["long long n", "long long *bytes"], [_ll, C.POINTER(_ll)]),
    "dlesm_particle_order_f64": (
        ["int xstart", "int xstop", "int ystart", "int ystop", "long long n", "const double *px", "const double *py",
         "const int *status", "int *perm", "int *nlive", "void *scratch", "long long scratch_bytes", "void *stream"],
        [_i] * 4 + [_ll] + [_vp] * 6 + [_ll, _vp]),
    "dlesm_particle_permute": (
        ["long long n", "const int *perm", "int narrays", "const void *const *src", "void *const *dst", "const int *elem_bytes",
         "void *stream"],
        [_ll, _vp, _i, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_i), _vp]),
    "dlesm_particle_sort_set": (["dlesm_drifters *set", "int xstart", "int xstop", "int ystart", "int ystop", "void *stream"],
                                [_vp, _i, _i, _i, _i, _vp]),
    "dlesm_particle_set_origin": (["dlesm_drifters *set", "int *origin", "long long *nlive"], [_vp, _vp, C.POINTER(_ll)]),
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
        assert "drifter" not in entry
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % entry, txt)
        assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == args, entry
        res, got = _cabi.PROTOTYPES[entry]
        assert res is C.c_int and list(got) == ctypes_args, entry
        m = re.search(r"`%s\(([^)]*)\)`" % entry, doc)
        assert m and [a.strip() for a in m.group(1).replace("\n", " ").split(",")] == _names(args), entry
        m = re.search(r"function %s\((.*?)\)\s*bind\(C, name=\"%s\"\)" % (entry, entry), fortran, flags=re.S)
        assert m and [a.strip() for a in m.group(1).replace("&", " ").split(",")] == _names(args), entry
    assert {e for e in exported[0] if "particle" in e} == set(ENTRIES)
    for name in ("psy.particle_order", "psy.particle_permute", "psy.particle_sort", "call particle_sort(set, un)",
                 "call particle_origin(set, origin, nlive)"):
        assert name in doc, name
    raw = open(os.path.join(ROOT, "include", "dlesm_hip.h")).read()
    assert "section 6.18" in raw
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 6.18 Particles in cell order (frozen here)" in design and all(e in design for e in ENTRIES)
    assert L.dlesm_version() == 310


def test_the_wrappers_are_public():
    from dl_esm_inf_amd import psy
    assert D.particle_order is psy.particle_order and D.particle_permute is psy.particle_permute
    assert D.particle_sort is psy.particle_sort
    sig = inspect.signature(psy.particle_order).parameters
    assert list(sig) == ["px", "py", "status", "grid", "perm", "stream"]
    assert sig["perm"].default is None and sig["stream"].default is None
    sig = inspect.signature(psy.particle_permute).parameters
    assert list(sig) == ["perm", "arrays", "out", "stream"] and sig["out"].default is None
    sig = inspect.signature(psy.particle_sort).parameters
    assert list(sig) == ["px", "py", "status", "un", "carry", "stream"] and sig["carry"].default == ()
    psy_f = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_psy_mod.f90")).read()
    for name, args in (("particle_sort", "set, un"), ("particle_origin", "set, origin, nlive")):
        assert re.search(r"public ::[^\n]*\b%s\b" % name, psy_f), name
        assert re.search(r"subroutine %s\(%s\)" % (name, re.escape(args)), psy_f), name
    assert "drifter_sample" not in psy_f


def test_the_scratch_query_is_host_arithmetic():
    """it needs no device; the bytes hold two key buffers, one value buffer and the 256 x nblocks table, and grow with n"""
    b = _ll(-3)
    assert L.dlesm_particle_order_scratch(-1, C.byref(b)) == _cabi.EINVAL and b.value == -3
    assert L.dlesm_particle_order_scratch(2 ** 31, C.byref(b)) == _cabi.EINVAL and b.value == -3
    assert L.dlesm_particle_order_scratch(1000, None) == _cabi.EINVAL
    last = -1
    for n in [0] + PC.NS + [2 ** 22, 2 ** 31 - 1]:
        assert L.dlesm_particle_order_scratch(n, C.byref(b)) == 0, n
        nblocks = -(-n // PC.TILE)
        assert b.value >= 12 * n + 4 * 256 * nblocks and b.value <= 12.5 * n + 4096 and b.value % 16 == 0, n
        assert b.value >= last
        last = b.value


def test_without_a_gpu_the_entries_fail_loudly_and_write_nothing():
    """DLESM_ENODEV without a device; with one, host arrays of a valid shape pass every check that needs no device and the
    bad arguments are refused"""
    n = 8
    px, py, st = np.full(n, 3.5), np.full(n, 4.5), np.zeros(n, dtype=np.int32)
    perm, nlive = np.full(n, -7, dtype=np.int32), np.full(1, -7, dtype=np.int32)
    need = _ll()
    assert L.dlesm_particle_order_scratch(n, C.byref(need)) == 0
    scratch = np.full(need.value // 8 + 2, -7.0)
    base = scratch.ctypes.data + (-scratch.ctypes.data) % 16
    have_gpu = L.dlesm_device_count() > 0
    want = _cabi.EINVAL if have_gpu else _cabi.ENODEV

    def order(box=(2, 7, 2, 7), n_=n, x=px.ctypes.data, pm=perm.ctypes.data, nl=nlive.ctypes.data, sc=base, nb=need.value):
        return L.dlesm_particle_order_f64(*box, n_, x, py.ctypes.data, st.ctypes.data, pm, nl, sc, nb, None)

    assert order(x=None) == want
    if not have_gpu:
        assert b"no HIP device" in L.dlesm_last_error()
        assert order() == _cabi.ENODEV                                       # a valid call: nothing to run it on
    assert order(pm=None) == want and order(sc=None) == want
    assert order(n_=-1) == want and order(n_=2 ** 31) == want
    assert order(box=(2, 0, 2, 7)) == want and order(box=(2, 7, 2, 0)) == want
    assert order(box=(1, 65536, 1, 65536)) == want and order(box=(1, 65535, 1, 65537)) == want
    assert order(nb=need.value - 1) == want
    assert order(x=px.ctypes.data + 4) == want and order(pm=perm.ctypes.data + 2) == want and order(sc=base + 8) == want
    assert order(pm=px.ctypes.data) == want and order(nl=perm.ctypes.data) == want and order(sc=px.ctypes.data) == want
    assert order(nl=base) == want

    src, dst = np.arange(n, dtype=np.float64), np.full(n, -7.0)
    idx = np.arange(n, dtype=np.int32)

    def gather(k=1, n_=n, pm=idx.ctypes.data, s=src.ctypes.data, d=dst.ctypes.data, eb=8):
        ps, pd, pe = (_vp * 8)(*[s] * 8), (_vp * 8)(*[d] + [None] * 7), (_i * 8)(*[eb] * 8)
        return L.dlesm_particle_permute(n_, pm, k, ps, pd, pe, None)

    if not have_gpu:
        assert gather() == _cabi.ENODEV
    assert gather(k=0) == want and gather(k=9) == want and gather(k=2) == want       # (k = 2: dst[1] is null)
    assert gather(n_=-1) == want and gather(n_=2 ** 31) == want and gather(pm=None) == want
    assert gather(eb=2) == want and gather(eb=16) == want
    assert gather(s=None) == want and gather(d=None) == want
    assert gather(d=src.ctypes.data) == want and gather(d=idx.ctypes.data, eb=4) == want
    assert gather(s=src.ctypes.data + 4) == want
    assert L.dlesm_particle_permute(n, idx.ctypes.data, 1, None, None, None, None) == want
    assert L.dlesm_particle_sort_set(None, 2, 7, 2, 7, None) == want
    assert L.dlesm_particle_set_origin(None, perm.ctypes.data, None) == want
    assert (px == 3.5).all() and (py == 4.5).all() and (st == 0).all() and (perm == -7).all() and (nlive == -7).all()
    assert (scratch == -7.0).all() and (dst == -7.0).all() and (src == np.arange(n)).all() and (idx == np.arange(n)).all()
