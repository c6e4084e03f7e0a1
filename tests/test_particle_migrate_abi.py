"""CPU tests of the boundary of the particle migration: the seven entries are exported from the
product and from the lab build and stand in the header, the ctypes table and INTEGRATION.md with one argument list each; none
of their names contains `particle`, `drifter`, `cell_bin` or `dispersal` (the ABI tests of sections 6.17-6.20 pin those
sets); the new status and the record are the same in the header, the ctypes module, the Fortran module and the restatement;
dlesm_version() is unchanged; the Python names are public; the three sizing functions are host arithmetic; without a GPU the
entries fail loudly and write nothing, and with one every refusal is DLESM_EINVAL with nothing written."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

import dl_esm_inf_amd as D
from dl_esm_inf_amd import _cabi

import particle_migrate_numpy as M

L = _cabi.lib()
_i, _vp, _ll, _pi = C.c_int, C.c_void_p, C.c_longlong, C.POINTER(C.c_int)
BOXARGS = ["int xstart", "int xstop", "int ystart", "int ystop"]
ENTRIES = {
    "dlesm_migrate_bytes": (["long long cap", "int npayload", "long long *bytes"], [_ll, _i, C.POINTER(_ll)]),
    "dlesm_migrate_scratch": (["long long n", "long long *bytes"], [_ll, C.POINTER(_ll)]),
    "dlesm_migrate_work": (["long long n", "long long cap", "int npayload", "long long *bytes"], [_ll, _ll, _i, C.POINTER(_ll)]),
    "dlesm_migrate_pack_f64": (
        ["int axis"] + BOXARGS + ["long long n", "const double *px", "const double *py", "int *status", "const long long *id",
                                  "const void *const *payload", "int npayload", "const int *has_neighbour", "const int *shift_x",
                                  "const int *shift_y", "long long cap", "void *const *send", "dlesm_migrate_counts *counts",
                                  "void *scratch", "long long scratch_bytes", "void *stream"],
        [_i] * 5 + [_ll] + [_vp] * 4 + [C.POINTER(_vp), _i, _pi, _pi, _pi, _ll, C.POINTER(_vp), _vp, _vp, _ll, _vp]),
    "dlesm_migrate_unpack_f64": (
        ["int axis"] + BOXARGS + ["long long n", "double *px", "double *py", "int *status", "long long *id",
                                  "void *const *payload", "int npayload", "long long cap", "const void *const *recv",
                                  "dlesm_migrate_counts *counts", "void *scratch", "long long scratch_bytes", "void *stream"],
        [_i] * 5 + [_ll] + [_vp] * 4 + [C.POINTER(_vp), _i, _ll, C.POINTER(_vp), _vp, _vp, _ll, _vp]),
    "dlesm_migrate_exchange": (["const int *neighbour", "const void *const *send", "void *const *recv", "long long bytes",
                                "void *stream"], [_pi, C.POINTER(_vp), C.POINTER(_vp), _ll, _vp]),
    "dlesm_migrate_f64": (
        BOXARGS + ["long long n", "double *px", "double *py", "int *status", "long long *id", "void *const *payload",
                   "int npayload", "const int *neighbour", "const int *shift_x", "const int *shift_y", "long long cap",
                   "dlesm_migrate_counts *counts", "void *work", "long long work_bytes", "void *stream"],
        [_i] * 4 + [_ll] + [_vp] * 4 + [C.POINTER(_vp), _i, _pi, _pi, _pi, _ll, _vp, _vp, _ll, _vp]),
}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dlesm_hip.h")).read(), flags=re.S)


def _names(args):
    return [a.split()[-1].lstrip("*") for a in args]


def test_header_exports_ctypes_and_documents_agree():
    txt = _header()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    exported = []
    for lib in [_cabi.LIB_PATH, os.path.join(os.path.dirname(_cabi.LIB_PATH), "libdlesm_hip_lab.so")]:
        out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
        exported.append({l.split()[-1] for l in out.splitlines() if " T " in l})
    for entry, (args, ctypes_args) in ENTRIES.items():
        assert entry in exported[0] and entry in exported[1], entry
        assert not any(w in entry for w in ("particle", "drifter", "cell_bin", "dispersal")), entry
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % entry, txt)
        assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == args, entry
        res, got = _cabi.PROTOTYPES[entry]
        assert res is C.c_int and list(got) == ctypes_args, entry
        m = re.search(r"`%s\(([^)]*)\)`" % entry, doc)
        assert m and [a.strip() for a in m.group(1).replace("\n", " ").split(",")] == _names(args), entry
    assert {e for e in exported[0] if "migrate" in e} == set(ENTRIES)
    for name in ("psy.particle_migrate", "psy.particle_pack", "psy.particle_unpack", "psy.particle_exchange",
                 "DLESM_DRIFTER_FREE", "dlesm_migrate_counts", "nsub = 1"):
        assert name in doc, name
    raw = open(os.path.join(ROOT, "include", "dlesm_hip.h")).read()
    assert "section 6.21" in raw
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 6.21 Particles that cross rank boundaries (frozen here)" in design and all(e in design for e in ENTRIES)
    assert L.dlesm_version() == 310


def test_the_numbers_and_the_record_agree():
    h = _header()
    assert re.search(r"enum\s*\{\s*DLESM_DRIFTER_FREE = 4\s*\}", h)
    assert re.search(r"enum\s*\{\s*DLESM_MIGRATE_MAX_PAYLOAD = 4\s*\}", h)
    assert re.search(r"enum\s*\{\s*DLESM_MIGRATE_W = 0,\s*DLESM_MIGRATE_E,\s*DLESM_MIGRATE_S,\s*DLESM_MIGRATE_N\s*\}", h)
    assert re.search(r"enum\s*\{\s*DLESM_MIGRATE_X = 0,\s*DLESM_MIGRATE_Y = 1\s*\}", h)
    assert _cabi.DRIFTER_FREE == M.FREE == 4 and _cabi.DRIFTER_GROUNDED == 3
    assert (_cabi.MIGRATE_W, _cabi.MIGRATE_E, _cabi.MIGRATE_S, _cabi.MIGRATE_N) == (M.W, M.E, M.S, M.N) == (0, 1, 2, 3)
    assert (_cabi.MIGRATE_X, _cabi.MIGRATE_Y) == (M.AXIS_X, M.AXIS_Y) == (0, 1)
    assert _cabi.MIGRATE_MAX_PAYLOAD == M.MAX_PAYLOAD == 4
    fortran = open(os.path.join(ROOT, "dl_esm_inf_amd", "fortran", "dlesm_hip_mod.f90")).read()
    assert re.search(r"DLESM_DRIFTER_GROUNDED = 3, DLESM_DRIFTER_FREE = 4\b", fortran)
    m = re.search(r"typedef struct dlesm_migrate_counts \{(.*?)\} dlesm_migrate_counts;", h, flags=re.S)
    assert m and [" ".join(f.split()) for f in m.group(1).split(";") if f.strip()] == [
        "int sent[4]", "int held[4]", "int arrived[4]", "int dropped", "int nfree", "int bad_message", "int pad"]
    assert C.sizeof(_cabi.MigrateCounts) == 64 == 4 * M.RECORD
    rec = _cabi.MigrateCounts.from_buffer_copy(np.arange(16, dtype=np.int32).tobytes())
    assert rec.as16() == tuple(range(16))
    assert (rec.dropped, rec.nfree, rec.bad_message, rec.pad) == (M.DROPPED, M.NFREE, M.BAD, M.PAD)


def test_the_wrappers_are_public():
    from dl_esm_inf_amd import psy
    for name in ("particle_migrate", "particle_pack", "particle_unpack", "particle_exchange", "migrate_message",
                 "migrate_neighbours", "MigrateError"):
        assert getattr(D, name) is getattr(psy, name), name
    sig = inspect.signature(psy.particle_migrate).parameters
    assert list(sig) == ["px", "py", "status", "ids", "grid_or_field", "payload", "cap", "work", "stream"]
    assert sig["payload"].default == () and sig["work"].default is None and sig["stream"].default is None
    assert issubclass(psy.MigrateError, D.DlesmError)


def test_the_sizing_functions_are_host_arithmetic():
    """none needs a device; a message is 16 + (3 + npayload) * 8 * cap bytes; the scratch holds the 2 x nblocks + 1 table, its
    sums and eight words a block, and grows with n; the work area holds eight messages and the scratch"""
    b = _ll(-3)
    for bad in ((0, 0), (-1, 0), (2 ** 31, 0), (10, -1), (10, 5)):
        assert L.dlesm_migrate_bytes(*bad, C.byref(b)) == _cabi.EINVAL and b.value == -3, bad
    assert L.dlesm_migrate_bytes(10, 0, None) == _cabi.EINVAL
    for cap in (1, 64, 100, 2 ** 31 - 1):
        for k in range(5):
            assert L.dlesm_migrate_bytes(cap, k, C.byref(b)) == 0 and b.value == 16 + (3 + k) * 8 * cap == 8 * M.message_words(cap, k)
    b.value = -3
    assert L.dlesm_migrate_scratch(-1, C.byref(b)) == _cabi.EINVAL and L.dlesm_migrate_scratch(2 ** 31, C.byref(b)) == _cabi.EINVAL
    assert L.dlesm_migrate_scratch(10, None) == _cabi.EINVAL and b.value == -3
    last = 0
    for n in [0, 1, 4096, 4097, 70001, M.first_multiblock_n(2) - 1, M.first_multiblock_n(2), 2 ** 24, 2 ** 31 - 1]:
        assert L.dlesm_migrate_scratch(n, C.byref(b)) == 0, n
        nblocks = -(-n // M.TILE)
        assert b.value >= 4 * (2 * nblocks + 1) + 32 * nblocks and b.value <= 44 * nblocks + 128 and b.value % 16 == 0, n
        assert b.value >= last > -1
        last = b.value
    w = _ll(-3)
    for bad in ((-1, 10, 0), (2 ** 31, 10, 0), (10, 0, 0), (10, 2 ** 31, 0), (10, 10, 5), (10, 10, -1)):
        assert L.dlesm_migrate_work(*bad, C.byref(w)) == _cabi.EINVAL and w.value == -3, bad
    assert L.dlesm_migrate_work(10, 10, 0, None) == _cabi.EINVAL
    for n, cap, k in ((0, 1, 0), (1000, 7, 3), (70001, 100, 4)):
        assert L.dlesm_migrate_work(n, cap, k, C.byref(w)) == 0 and L.dlesm_migrate_scratch(n, C.byref(b)) == 0
        msg = -(-(16 + (3 + k) * 8 * cap) // 16) * 16
        assert w.value == 8 * msg + b.value


def test_without_a_gpu_the_entries_fail_loudly_and_write_nothing():
    """DLESM_ENODEV without a device; with one, host arrays of a valid shape pass every check that needs no device and the
    bad arguments are refused"""
    n, cap, k = 8, 4, 2
    px, py, st = np.full(n, 3.5), np.full(n, 4.5), np.full(n, 1, dtype=np.int32)
    ids, pay = np.arange(n, dtype=np.int64), [np.full(n, 7, dtype=np.int64) for _ in range(k)]
    words = M.message_words(cap, k)
    msgs = [np.full(words + 2, -7, dtype=np.int64) for _ in range(4)]
    mp = [m.ctypes.data + (-m.ctypes.data) % 16 for m in msgs]
    counts = np.full(16, -7, dtype=np.int32)
    need, wneed = _ll(), _ll()
    assert L.dlesm_migrate_scratch(n, C.byref(need)) == 0 and L.dlesm_migrate_work(n, cap, k, C.byref(wneed)) == 0
    scratch, work = np.full(need.value // 8 + 2, -7.0), np.full(wneed.value // 8 + 2, -7.0)
    base, wbase = scratch.ctypes.data + (-scratch.ctypes.data) % 16, work.ctypes.data + (-work.ctypes.data) % 16
    have_gpu = L.dlesm_device_count() > 0
    want = _cabi.EINVAL if have_gpu else _cabi.ENODEV
    two, four = (C.c_int * 2)(1, 1), (C.c_int * 4)(-1, -1, -1, -1)

    def pack(axis=0, box=(2, 7, 2, 7), n_=n, x=px.ctypes.data, s=st.ctypes.data, i=ids.ctypes.data, p0=pay[0].ctypes.data, k_=k,
             has=two, cap_=cap, m0=mp[0], m1=mp[1], c=counts.ctypes.data, sc=base, nb=need.value, msgs_=True):
        pp = (_vp * 4)(p0, pay[1].ctypes.data, None, None)
        return L.dlesm_migrate_pack_f64(axis, *box, n_, x, py.ctypes.data, s, i, pp, k_, has, two, two, cap_,
                                        (_vp * 2)(m0, m1) if msgs_ else None, c, sc, nb, None)

    def unpack(axis=0, n_=n, x=px.ctypes.data, k_=k, cap_=cap, m0=mp[2], m1=mp[3], c=counts.ctypes.data, sc=base, nb=need.value):
        pp = (_vp * 4)(pay[0].ctypes.data, pay[1].ctypes.data, None, None)
        return L.dlesm_migrate_unpack_f64(axis, 2, 7, 2, 7, n_, x, py.ctypes.data, st.ctypes.data, ids.ctypes.data, pp, k_, cap_,
                                          (_vp * 2)(m0, m1), c, sc, nb, None)

    def whole(n_=n, x=px.ctypes.data, k_=k, cap_=cap, nb4=four, c=counts.ctypes.data, w=wbase, wb=wneed.value):
        pp = (_vp * 4)(pay[0].ctypes.data, pay[1].ctypes.data, None, None)
        return L.dlesm_migrate_f64(2, 7, 2, 7, n_, x, py.ctypes.data, st.ctypes.data, ids.ctypes.data, pp, k_, nb4, four, four,
                                   cap_, c, w, wb, None)

    assert pack(x=None) == want
    if not have_gpu:
        assert b"no HIP device" in L.dlesm_last_error()
        assert pack() == unpack() == whole() == _cabi.ENODEV                # valid calls: nothing to run them on
    for call in (pack, unpack, whole):
        assert call(x=None) == want and call(n_=-1) == want and call(n_=2 ** 31) == want
        assert call(cap_=0) == want and call(cap_=2 ** 31) == want and call(k_=-1) == want and call(k_=5) == want
        assert call(k_=3) == want                                            # payload[2] is null
        assert call(x=px.ctypes.data + 4) == want and call(c=None) == want and call(c=counts.ctypes.data + 2) == want
    assert unpack(x=py.ctypes.data) == want and whole(x=py.ctypes.data) == want      # both write px and py
    assert pack(axis=2) == want and pack(axis=-1) == want and unpack(axis=2) == want
    assert pack(box=(2, 0, 2, 7)) == want and pack(box=(2, 7, 2, 0)) == want
    assert pack(s=None) == want and pack(i=None) == want and pack(s=st.ctypes.data + 2) == want and pack(i=ids.ctypes.data + 4) == want
    assert pack(p0=pay[0].ctypes.data + 4) == want and pack(has=None) == want and pack(msgs_=False) == want
    assert pack(m0=None) == want and pack(m1=mp[1] + 8) == want and pack(sc=None) == want and pack(sc=base + 8) == want
    assert pack(nb=need.value - 1) == want and unpack(nb=need.value - 1) == want and unpack(sc=base + 8) == want
    assert pack(m0=mp[1]) == want and pack(m0=px.ctypes.data) == want and pack(m1=ids.ctypes.data) == want     # overlaps
    assert pack(sc=mp[0]) == want and pack(c=mp[0]) == want and pack(s=mp[1]) == want and pack(m0=pay[1].ctypes.data) == want
    assert unpack(m0=px.ctypes.data) == want and unpack(c=mp[2]) == want and unpack(sc=mp[3]) == want
    assert whole(w=None) == want and whole(w=wbase + 8) == want and whole(wb=wneed.value - 1) == want and whole(nb4=None) == want
    assert whole(w=px.ctypes.data) == want and whole(c=wbase) == want
    # the transport's own refusals need no device
    sends, recvs = (_vp * 2)(mp[0], mp[1]), (_vp * 2)(mp[2], mp[3])
    nbytes = 8 * words
    assert L.dlesm_migrate_exchange(None, sends, recvs, nbytes, None) == _cabi.EINVAL
    assert L.dlesm_migrate_exchange(two, None, recvs, nbytes, None) == _cabi.EINVAL
    assert L.dlesm_migrate_exchange(two, sends, None, nbytes, None) == _cabi.EINVAL
    assert L.dlesm_migrate_exchange(two, sends, recvs, 8, None) == _cabi.EINVAL
    assert L.dlesm_migrate_exchange(two, sends, recvs, nbytes + 4, None) == _cabi.EINVAL
    assert L.dlesm_migrate_exchange(two, sends, recvs, nbytes, None) == _cabi.EINVAL       # rank 1 of one rank
    assert L.dlesm_migrate_exchange((C.c_int * 2)(-1, -1), sends, sends, nbytes, None) == _cabi.EINVAL
    assert L.dlesm_migrate_exchange((C.c_int * 2)(-1, -1), sends, (_vp * 2)(mp[2], mp[2]), nbytes, None) == _cabi.EINVAL
    assert L.dlesm_migrate_exchange((C.c_int * 2)(-1, -1), sends, (_vp * 2)(mp[2], mp[3] + 8), nbytes, None) == _cabi.EINVAL
    assert (px == 3.5).all() and (py == 4.5).all() and (st == 1).all() and (ids == np.arange(n)).all()
    assert all((p == 7).all() for p in pay) and all((m == -7).all() for m in msgs) and (counts == -7).all()
    assert (scratch == -7.0).all() and (work == -7.0).all()
