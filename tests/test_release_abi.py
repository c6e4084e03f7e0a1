"""CPU tests of the boundary of the particle release: the two entries are exported from the product
and from the lab build and stand in the header, the ctypes table and INTEGRATION.md with one argument list each, and no other
export contains `release`; the two structures are 64 bytes with their members where the header puts them, through a C compiler
and through ctypes; dlesm_release_scratch is host arithmetic, monotone in n, and refuses what the rule refuses; dlesm_version()
is unchanged; the Python names are public; without a GPU the entry fails loudly and writes nothing."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

from conftest import ROOT

import dl_esm_inf_amd as D
from dl_esm_inf_amd import _cabi

import release_numpy as R

L = _cabi.lib()
_i, _vp, _ll = C.c_int, C.c_void_p, C.c_longlong
ENTRIES = {
    "dlesm_release_scratch": (["long long n", "int nsources", "int max_count", "long long *bytes"], [_ll, _i, _i, C.POINTER(_ll)]),
    "dlesm_release_f64": (
        ["int ld", "int ny", "int xstart", "int xstop", "int ystart", "int ystop", "int offx", "int offy", "const int *tmask",
         "dlesm_release_source *sources", "int nsources", "int max_count", "long long seed", "long long tick",
         "const long long *tick_dev", "long long n", "double *px", "double *py", "int *status", "long long *id", "long long *tag",
         "long long *born", "dlesm_release_counts *counts", "void *scratch", "long long scratch_bytes", "void *stream"],
        [_i] * 8 + [_vp, _vp, _i, _i, _ll, _ll, _vp, _ll] + [_vp] * 8 + [_ll, _vp]),
}
SOURCE = [("x", 0), ("y", 8), ("rx", 16), ("ry", 24), ("next_id", 32), ("count", 40), ("tag", 48), ("pad", 56)]
COUNTS = [("requested", 0), ("released", 8), ("foreign", 12), ("on_land", 16), ("dropped", 20), ("edge", 24), ("nfree", 28),
          ("clamped", 32), ("bad_source", 36), ("pad", 40)]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dlesm_hip.h")).read(), flags=re.S)


def test_header_exports_ctypes_and_documents_agree():
    txt = _header()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for lib in [_cabi.LIB_PATH, os.path.join(os.path.dirname(_cabi.LIB_PATH), "libdlesm_hip_lab.so")]:
        out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
        assert {e for e in exported if "release" in e} == set(ENTRIES), lib
    for entry, (args, ctypes_args) in ENTRIES.items():
        assert not any(w in entry for w in ("particle", "drifter", "cell_bin", "dispersal", "random_walk", "migrate")), entry
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % entry, txt)
        assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == args, entry
        res, got = _cabi.PROTOTYPES[entry]
        assert res is C.c_int and list(got) == ctypes_args, entry
        m = re.search(r"`%s\(([^)]*)\)`" % entry, doc)
        assert m and [a.strip() for a in m.group(1).replace("\n", " ").split(",")] == [a.split()[-1].lstrip("*") for a in args], entry
    assert {p for p in _cabi.PROTOTYPES if "release" in p} == set(ENTRIES)
    for name in ("psy.particle_release", "psy.release_sources", "psy.ReleaseError", "dlesm_release_source", "dlesm_release_counts",
                 "DLESM_RELEASE_MAX_SOURCES"):
        assert name in doc, name
    assert "section 6.23" in open(os.path.join(ROOT, "include", "dlesm_hip.h")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 6.23 Particle sources that fill FREE slots (frozen here)" in design and all(e in design for e in ENTRIES)
    assert "dlesm_release_f64" in design[design.index("## 10. Out of scope"):]
    assert "dlesm_release_f64" in open(os.path.join(ROOT, "README.md")).read()
    assert L.dlesm_version() == 310


def test_the_structures_are_64_bytes_with_the_members_at_the_headers_offsets():
    h = _header()
    assert re.search(r"enum\s*\{\s*DLESM_RELEASE_MAX_SOURCES = 65536\s*\}", h) and _cabi.RELEASE_MAX_SOURCES == 65536
    m = re.search(r"typedef struct dlesm_release_source \{(.*?)\} dlesm_release_source;", h, flags=re.S)
    assert m and [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()] == [
        "double x, y", "double rx, ry", "long long next_id", "long long count", "long long tag", "long long pad"]
    m = re.search(r"typedef struct dlesm_release_counts \{(.*?)\} dlesm_release_counts;", h, flags=re.S)
    assert m and [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()] == [
        "long long requested", "int released, foreign, on_land, dropped, edge, nfree, clamped, bad_source", "int pad[6]"]
    for cls, members in ((_cabi.ReleaseSource, SOURCE), (_cabi.ReleaseCounts, COUNTS)):
        assert C.sizeof(cls) == 64
        assert [(n, getattr(cls, n).offset) for n, _ in cls._fields_] == members
    # the restatement's record and table are the same words
    assert [o // 4 for _, o in COUNTS[:9]] == [R.REQUESTED, R.RELEASED, R.FOREIGN, R.ON_LAND, R.DROPPED, R.EDGE, R.NFREE,
                                               R.CLAMPED, R.BAD_SOURCE]
    assert [o // 8 for _, o in SOURCE] == [R.X, R.Y, R.RX, R.RY, R.NEXT_ID, R.COUNT, R.TAG, R.PAD]
    rec = _cabi.ReleaseCounts.from_buffer_copy(R.record(2 ** 40 + 5, 1, 2, 3, 4, 5, 6, 7, 8).tobytes())
    assert (rec.requested, rec.released, rec.foreign, rec.on_land, rec.dropped, rec.edge, rec.nfree, rec.clamped,
            rec.bad_source, list(rec.pad)) == (2 ** 40 + 5, 1, 2, 3, 4, 5, 6, 7, 8, [0] * 6)
    cc = shutil.which("cc") or shutil.which("gcc")            # the same through a C compiler, where there is one
    if cc:
        src = ('#include <stddef.h>\n#include <stdio.h>\n#include "dlesm_hip.h"\nint main(void){'
               'printf("%zu", sizeof(dlesm_release_source));' +
               "".join('printf(" %%zu", offsetof(dlesm_release_source, %s));' % n for n, _ in SOURCE) +
               'printf(" %zu", sizeof(dlesm_release_counts));' +
               "".join('printf(" %%zu", offsetof(dlesm_release_counts, %s));' % n for n, _ in COUNTS) + "return 0;}\n")
        with tempfile.TemporaryDirectory() as tmp:
            open(os.path.join(tmp, "t.c"), "w").write(src)
            subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "t.c"), "-o", os.path.join(tmp, "t")])
            out = subprocess.check_output([os.path.join(tmp, "t")], text=True).split()
        assert [int(v) for v in out] == [64] + [o for _, o in SOURCE] + [64] + [o for _, o in COUNTS]


def test_the_wrappers_are_public():
    from dl_esm_inf_amd import psy
    for name in ("particle_release", "release_sources", "ReleaseError"):
        assert getattr(D, name) is getattr(psy, name), name
    sig = inspect.signature(psy.particle_release).parameters
    assert list(sig) == ["sources", "px", "py", "status", "ids", "grid_or_field", "seed", "tick", "tick_dev", "tag", "born",
                         "max_count", "scratch", "stream", "wait"]
    assert sig["tick"].default == 0 and sig["wait"].default is True and sig["max_count"].default is None
    sig = inspect.signature(psy.release_sources).parameters
    assert list(sig) == ["x", "y", "rx", "ry", "first_id", "count", "tag", "device"]
    assert sig["count"].default == 0 and sig["tag"].default is None and sig["device"].default == "cuda"
    assert issubclass(psy.ReleaseError, D.DlesmError)


def test_the_scratch_size_is_host_arithmetic():
    """no device needed; monotone in n; it holds the table of 4 x candidate blocks + slot blocks + 1 counts, four words a block
    of either kind and min(n, nsources x max_count) staged records of 36 bytes"""
    b = _ll(-3)
    bad = [(-1, 1, 1), (2 ** 31, 1, 1), (10, -1, 1), (10, 65537, 1), (10, 1, 0), (10, 1, -5), (10, 65536, 32768),
           (10, 3, 2 ** 30), (10, 2 ** 14 + 1, 2 ** 16), (10, 65536, 16385)]
    for args in bad:
        assert L.dlesm_release_scratch(*args, C.byref(b)) == _cabi.EINVAL and b.value == -3, args
        assert b"dlesm_release_scratch" in L.dlesm_last_error()
    assert L.dlesm_release_scratch(10, 1, 1, None) == _cabi.EINVAL
    for ns, mc in ((0, 1), (1, 1), (15, 256), (15, 1000), (2100, 1), (65536, 16384), (1, 2 ** 30), (2 ** 14, 2 ** 16)):
        last = 0
        for n in [0, 1, 64, 4095, 4096, 4097, 12289, 2 ** 20, 2 ** 24, 2 ** 31 - 1]:
            assert L.dlesm_release_scratch(n, ns, mc, C.byref(b)) == 0, (n, ns, mc)
            ncand, nblocks, cap = ns * -(-mc // R.CHUNK), -(-n // R.TILE), min(n, ns * mc)
            least = 4 * (4 * ncand + nblocks + 1) + 16 * (ncand + nblocks) + 36 * cap
            assert least <= b.value <= least + 4 * (-(-(4 * ncand + nblocks + 1) // R.SCAN_TILE)) + 128 and b.value % 16 == 0
            assert b.value >= last
            last = b.value


def test_without_a_gpu_the_entry_fails_loudly_and_writes_nothing():
    """DLESM_ENODEV without a device; with one, host arrays of a valid shape pass every check that needs no device and the bad
    arguments are refused"""
    n, ns, mc = 8, 2, 4
    px, py, st = np.full(n, 3.5), np.full(n, 4.5), np.full(n, 4, dtype=np.int32)
    ids, tag, born = (np.full(n, 7, dtype=np.int64) for _ in range(3))
    tm = np.ones((9, 10), dtype=np.int32)
    src = R.table([3.5, 4.5], [3.5, 4.5], [1.0, 0.0], [1.0, 0.0], [0, 100], [3, 4])
    src0 = src.copy()
    counts = np.full(16, -7, dtype=np.int32)
    need = _ll()
    assert L.dlesm_release_scratch(n, ns, mc, C.byref(need)) == 0
    scratch = np.full(need.value // 8 + 2, -7.0)
    base = scratch.ctypes.data + (-scratch.ctypes.data) % 16
    have_gpu = L.dlesm_device_count() > 0
    want = _cabi.EINVAL if have_gpu else _cabi.ENODEV

    def call(box=(2, 9, 2, 8), ld=10, ny=9, t=tm.ctypes.data, s=src.ctypes.data, ns_=ns, mc_=mc, tick=0, n_=n, x=px.ctypes.data,
             y=py.ctypes.data, st_=st.ctypes.data, i=ids.ctypes.data, tg=tag.ctypes.data, bn=born.ctypes.data,
             c=counts.ctypes.data, sc=base, nb=need.value):
        return L.dlesm_release_f64(ld, ny, *box, 0, 0, t, s, ns_, mc_, 1, tick, None, n_, x, y, st_, i, tg, bn, c, sc, nb, None)

    assert call(x=None) == want
    if not have_gpu:
        assert b"no HIP device" in L.dlesm_last_error()
        assert call() == _cabi.ENODEV                                       # a valid call: nothing to run it on
    for kw in (dict(t=None), dict(s=None), dict(x=None), dict(y=None), dict(st_=None), dict(i=None), dict(c=None), dict(sc=None),
               dict(x=px.ctypes.data + 4), dict(i=ids.ctypes.data + 4), dict(tg=tag.ctypes.data + 4), dict(bn=born.ctypes.data + 4),
               dict(s=src.ctypes.data + 4), dict(st_=st.ctypes.data + 2), dict(t=tm.ctypes.data + 2), dict(sc=base + 8),
               dict(n_=-1), dict(n_=2 ** 31), dict(ns_=-1), dict(ns_=65537), dict(mc_=0), dict(mc_=2 ** 31 - 1), dict(tick=-1),
               dict(box=(1, 9, 2, 8)), dict(box=(2, 10, 2, 8)), dict(box=(2, 9, 2, 9)), dict(ld=0), dict(nb=need.value - 1),
               dict(y=px.ctypes.data), dict(i=px.ctypes.data), dict(tg=ids.ctypes.data), dict(bn=tag.ctypes.data),
               dict(c=src.ctypes.data), dict(sc=px.ctypes.data - px.ctypes.data % 16), dict(t=st.ctypes.data),
               dict(s=tm.ctypes.data), dict(c=tm.ctypes.data + 8)):
        assert call(**kw) == want, kw
    assert (px == 3.5).all() and (py == 4.5).all() and (st == 4).all() and all((a == 7).all() for a in (ids, tag, born))
    assert (src == src0).all() and (counts == -7).all() and (scratch == -7.0).all() and (tm == 1).all()
