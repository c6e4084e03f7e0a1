"""GPU tests (-m gpu) of the particle release: px, py, status, id, tag, born, the whole source table
and the 64-byte record after dlesm_release_f64 equal the restatements (tests/release_numpy.py) bit for bit on the shared cases
(tests/release_cases.py) -- three offsets, seven slot counts, five FREE patterns, counts around the chunk of 256 with both
max_counts, every kind of source, more accepted than FREE, the rounding edge, a candidate table and a slot table deep enough
for the three-kernel scan, tag and born given and NULL.  Every array is filled with a sentinel first and has guard elements
behind it, so every word the rule does not name is checked.  Two calls continue the ids; the tiles of 2 x 2 and 3 x 2
decompositions, each with arrays of its own, release between them the undivided device run; a captured graph of a release and
a dispersal step replayed three times equals three eager iterations; every refusal returns DLESM_EINVAL and changes nothing;
the Python wrapper.  Everything is an integer or a bit pattern: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import particle_migrate_numpy as M
import release_cases as RC
import release_numpy as R

pytestmark = pytest.mark.gpu
SLACK, GUARD, BYTE_FILL = 8, 256, 0xA5
CASES = RC.cases()


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    import dl_esm_inf_amd as d
    torch.cuda.set_device(0)
    d.parallel_init(0, 1)
    yield torch, d, d._cabi.lib()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _guarded(torch, a, fill):
    """a host array on the device with SLACK guard elements (rows) behind it"""
    tail = np.full((SLACK,) + a.shape[1:], fill, dtype=a.dtype)
    return torch.from_numpy(np.concatenate([a, tail])).cuda()


class Dev:
    """a case on the device: its arrays before the call, the table, the record, the mask, the scratch with guard bytes"""

    def __init__(self, torch, L, c, tm=None, arr=None):
        self.c, self.n = c, c["n"]
        host = RC.arrays(c) if arr is None else arr
        self.fills = [RC.SENT_F, RC.SENT_F, -9, RC.SENT_I, RC.SENT_I, RC.SENT_I]
        self.arr = [None if a is None else _guarded(torch, a, f) for a, f in zip(host, self.fills)]
        self.src = _guarded(torch, c["sources"], RC.SENT_I)
        self.ns = len(c["sources"])
        self.counts = torch.full((16 + SLACK,), -9, dtype=torch.int32, device="cuda")
        self.tm = torch.from_numpy(np.ascontiguousarray(RC.mask() if tm is None else tm)).cuda()
        b = C.c_longlong(-1)
        assert L.dlesm_release_scratch(self.n, self.ns, c["max_count"], C.byref(b)) == 0 and b.value > 0
        self.need = b.value
        self.scratch = torch.full((self.need + GUARD,), BYTE_FILL, dtype=torch.uint8, device="cuda")
        self.tick_dev = torch.full((1,), RC.TICK_DEV, dtype=torch.int64, device="cuda") if c["optional"] else None

    def call(self, L, stream=None, tick=RC.TICK, **kw):
        c = self.c
        a = dict(ld=self.tm.shape[1], ny=self.tm.shape[0], box=c["box"], off=c["off"], tm=self.tm.data_ptr(),
                 src=self.src.data_ptr(), ns=self.ns, mc=c["max_count"], seed=c["seed"], tick=tick,
                 td=self.tick_dev.data_ptr() if self.tick_dev is not None else None, n=self.n,
                 arr=[t.data_ptr() if t is not None else None for t in self.arr], counts=self.counts.data_ptr(),
                 sc=self.scratch.data_ptr(), nb=self.need)
        a.update(kw)
        seed = a["seed"] & R.MASK64
        return L.dlesm_release_f64(a["ld"], a["ny"], *a["box"], *a["off"], C.c_void_p(a["tm"]), C.c_void_p(a["src"]), a["ns"],
                                   a["mc"], seed - (1 << 64) if seed >> 63 else seed, a["tick"], C.c_void_p(a["td"]), a["n"],
                                   *[C.c_void_p(p) for p in a["arr"]], C.c_void_p(a["counts"]), C.c_void_p(a["sc"]), a["nb"],
                                   C.c_void_p(stream.cuda_stream) if stream is not None else None)

    def tensors(self):
        return [t for t in self.arr if t is not None] + [self.src, self.counts, self.scratch, self.tm] + \
            ([self.tick_dev] if self.tick_dev is not None else [])

    def host(self):
        return [None if t is None else t.cpu().numpy() for t in self.arr], self.src.cpu().numpy(), self.counts.cpu().numpy()

    def check(self, want, what):
        """every word of every array, the table and the record against (arrays, table, record), and the guards"""
        warr, wsrc, wrec = want
        arr, src, counts = self.host()
        names = ("px", "py", "status", "id", "tag", "born")
        for k, (g, w) in enumerate(zip(arr, warr)):
            assert (g is None) == (w is None)
            if g is not None:
                assert g[:self.n].tobytes() == w.tobytes(), (what, names[k], np.flatnonzero(g[:self.n] != w)[:8])
                assert (g[self.n:] == self.fills[k]).all(), (what, names[k], "guard")
        assert (src[:self.ns] == wsrc).all() and (src[self.ns:] == RC.SENT_I).all(), (what, "sources")
        assert (counts[:16] == wrec).all() and (counts[16:] == -9).all(), (what, counts[:16], wrec)
        assert (self.scratch[self.need:] == BYTE_FILL).all().item(), (what, "behind the scratch")
        if self.tick_dev is not None:
            assert self.tick_dev.item() == RC.TICK_DEV, what
        return arr, src, counts


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c["name"].replace(" ", "_") for c in CASES])
def test_every_word_equals_the_restatements(T, k):
    torch, D, L = T
    c = CASES[k]
    d = Dev(torch, L, c)
    tm0 = d.tm.clone()
    assert d.call(L) == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    arr, src, counts = d.check(RC.reference(c), c["name"])
    assert R.invariant(counts[:16]) and torch.equal(d.tm, tm0)
    if k % 7 == 0:                                                    # the loop over candidates, on some
        d.check(RC.run(c, R.release_scalar), c["name"] + " (scalar)")


def test_the_cases_reach_every_path():
    recs = {c["name"]: RC.reference(c)[2] for c in CASES}
    assert recs["edge"][R.EDGE] == 1 and recs["overflow"][R.DROPPED] > 0 and recs["overflow"][R.NFREE] == 0
    assert 4 * 2100 + 2 + 1 > R.SCAN_TILE and R.requested(recs["deep table"]) == 2100 and recs["deep table"][R.RELEASED] > 500
    assert R.requested(recs["no sources"]) == 0 and recs["no sources"][R.NFREE] == 65
    assert recs["empty box"][R.FOREIGN] == R.requested(recs["empty box"]) > 0
    for c in CASES[:6]:
        r = recs[c["name"]]
        assert min(r[R.RELEASED], r[R.FOREIGN], r[R.ON_LAND], r[R.BAD_SOURCE]) > 0 and r[R.DROPPED] == 0, (c["name"], r)
    assert any(r[R.CLAMPED] > 0 for r in recs.values())
    assert sum(r[R.DROPPED] > 0 and r[R.RELEASED] > 0 for r in recs.values()) >= 5


def test_a_slot_table_deeper_than_one_scan_block(T):
    torch, D, L = T
    c = RC.deep_slots_case()
    assert -(-c["n"] // R.TILE) + 1 > R.SCAN_TILE
    d = Dev(torch, L, c)
    assert d.call(L) == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    want = RC.run(c)
    assert want[2][R.RELEASED] == 66 and want[2][R.DROPPED] > 0 and want[0][2][-1] != R.FREE
    d.check(want, c["name"])


def test_two_calls_continue_the_ids(T):
    """a then b gives the (id, position) set of a + b at once; without tick_dev, born is tick"""
    torch, D, L = T
    a, b = 100, 156
    c = RC.case("split", off=RC.OFFSETS[1], n=12289, pattern="all", max_count=256, src=RC.sources(RC.OFFSETS[1], counts=[a + b]))
    whole = Dev(torch, L, c)
    assert whole.call(L) == 0, L.dlesm_last_error()
    parts = Dev(torch, L, c)
    parts.tick_dev = None
    want = RC.arrays(c)
    wsrc = c["sources"].copy()
    for tick, k in ((3, a), (4, b)):
        parts.src[:parts.ns, R.COUNT] = torch.where(parts.src[:parts.ns, R.COUNT] >= 0, k, -1)
        wsrc[:, R.COUNT] = np.where(wsrc[:, R.COUNT] >= 0, k, -1)
        assert parts.call(L, tick=tick) == 0, L.dlesm_last_error()
        rec = R.release_vector(c["box"], c["off"], RC.mask(), wsrc, 256, c["seed"], tick, *want)
    torch.cuda.synchronize()
    arr, src, counts = parts.check((want, wsrc, rec), "two calls")
    assert set(np.unique(arr[5][:c["n"]]).tolist()) == {RC.SENT_I, 3, 4}
    warr = whole.host()[0]
    got, all_at_once = RC.census([t[:c["n"]] for t in arr], c["off"]), RC.census([t[:c["n"]] for t in warr], c["off"])
    assert got == all_at_once and len(got) > 500
    assert (src[:parts.ns, R.NEXT_ID] == whole.host()[1][:parts.ns, R.NEXT_ID]).all()


@pytest.mark.parametrize("mesh", [(2, 2), (3, 2)])
def test_the_tiles_release_the_undivided_device_run(T, mesh):
    torch, D, L = T
    tm, count = RC.basin_mask(), 300
    src = RC.basin_sources(count)

    def on_device(tile):
        c = RC.tile_case(tile, src, count)
        w = M.window(tm, tile)
        d = Dev(torch, L, c, tm=w)
        assert d.call(L) == 0, L.dlesm_last_error()
        torch.cuda.synchronize()
        arr, table, counts = d.check(RC.run(c, tm=w), ("tile", tile["off"]))
        return RC.census([t[:c["n"]] for t in arr], tile["off"]), table[:len(src)], counts[:16]

    want, after, rec = on_device(M.make_tiles(*RC.BASIN, 1, 1)[0])
    assert len(want) == rec[R.RELEASED] > 1000 and rec[R.ON_LAND] > 0 and rec[R.FOREIGN] > 0
    got = {}
    for t in M.make_tiles(*RC.BASIN, *mesh):
        mine, tafter, trec = on_device(t)
        assert (tafter == after).all() and trec[R.DROPPED] == 0
        assert not set(mine) & set(got), "a particle was released on two tiles"
        got.update(mine)
    assert got == want


def test_a_captured_graph_equals_eager_iterations(T):
    """{release, dispersal step with the device counter} three times: every replay releases fresh ids, is born at the counter's
    tick and moves with fresh kicks"""
    torch, D, L = T
    c = RC.case("graph", off=RC.OFFSETS[1], n=4097, pattern="third", max_count=256, src=RC.sources(RC.OFFSETS[1], counts=[40, 7]))
    ld, ny = RC.LD, RC.NY
    flow = [torch.full((ny, ld), v, dtype=torch.float64, device="cuda") for v in (1000.0, 1000.0, 0.3, -0.2)]

    def iteration(d, stream=None):
        rc = d.call(L, stream=stream)
        if rc == 0:
            rc = L.dlesm_dispersal_step_f64(250.0, 2, 5.0, 12345, 0, _ptr(d.tick_dev), ld, ny, *c["box"], _ptr(d.tm),
                                            *[_ptr(f) for f in flow], d.n, None, *[_ptr(t) for t in d.arr[:3]],
                                            C.c_void_p(stream.cuda_stream) if stream is not None else None)
        return rc

    eager = Dev(torch, L, c)
    for _ in range(3):
        assert iteration(eager) == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    g = Dev(torch, L, c)
    start = [t.clone() for t in g.tensors()]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        rc = iteration(g, stream=s)
    assert rc == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(g.tensors()[:-2], start[:-2])) and g.tick_dev.item() == RC.TICK_DEV    # not run
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(g.tensors(), eager.tensors()):
        if a is not g.scratch:
            assert torch.equal(a, b)
    assert g.tick_dev.item() == RC.TICK_DEV + 6
    born = g.arr[5][:g.n].cpu().numpy()
    assert set(np.unique(born).tolist()) == {RC.SENT_I} | {RC.TICK + RC.TICK_DEV + 2 * k for k in range(3)}
    # the eager run is three releases of the restatement as far as the release alone decides it: the ids and the table
    want, wsrc = RC.arrays(c), c["sources"].copy()
    for k in range(3):
        R.release_vector(c["box"], c["off"], RC.mask(), wsrc, 256, c["seed"], RC.TICK + RC.TICK_DEV + 2 * k, *want)
    assert (g.src[:g.ns].cpu().numpy() == wsrc).all() and (g.arr[3][:g.n].cpu().numpy() == want[3]).all()
    assert (g.arr[4][:g.n].cpu().numpy() == want[4]).all() and (born == want[5]).all()


def test_every_refusal_returns_einval_and_changes_nothing(T):
    torch, D, L = T
    EINVAL = D._cabi.EINVAL
    c = RC.case("refusals", off=RC.OFFSETS[1], n=4097, pattern="third", max_count=256)
    d = Dev(torch, L, c)
    before = [t.clone() for t in d.tensors()]
    p = [t.data_ptr() for t in d.arr]
    n, ns = d.n, d.ns

    def arr(k, v):
        return dict(arr=p[:k] + [v] + p[k + 1:])

    bad = [dict(tm=None), dict(src=None), dict(counts=None), dict(sc=None)]
    bad += [arr(k, None) for k in range(4)]                                             # tag and born may be null
    bad += [arr(k, p[k] + 4) for k in (0, 1, 3, 4, 5)] + [arr(2, p[2] + 2)]             # alignment
    bad += [dict(src=d.src.data_ptr() + 4), dict(td=d.tick_dev.data_ptr() + 4), dict(tm=d.tm.data_ptr() + 2),
            dict(counts=d.counts.data_ptr() + 4), dict(sc=d.scratch.data_ptr() + 8)]
    bad += [dict(n=-1), dict(n=2 ** 31), dict(ns=-1), dict(ns=65537), dict(mc=0), dict(mc=-1), dict(mc=2 ** 31 - 1),
            dict(ns=2 ** 14 + 1, mc=2 ** 16), dict(tick=-1), dict(nb=d.need - 1), dict(nb=-1)]
    bad += [dict(box=b) for b in ((1, 17, 4, 14), (5, 24, 4, 14), (5, 17, 1, 14), (5, 17, 4, 19))] + [dict(ld=0), dict(ny=0),
                                                                                                      dict(ld=17)]
    for k in range(6):                                                                  # a written array in any other array
        for q in range(6):
            if q != k:
                bad.append(arr(k, p[q]))
        bad += [arr(k, d.src.data_ptr()), arr(k, d.tm.data_ptr()), arr(k, d.scratch.data_ptr())]
    bad += [dict(src=p[0]), dict(src=d.tm.data_ptr()), dict(counts=p[3] + 8 * (n - 1)), dict(counts=d.src.data_ptr() + 64 * (ns - 1)),
            dict(counts=d.tm.data_ptr()), dict(sc=p[1]), dict(sc=d.tm.data_ptr()), dict(td=p[0]), dict(td=d.src.data_ptr() + 8),
            dict(td=d.counts.data_ptr() + 8), dict(td=d.scratch.data_ptr() + 16), dict(counts=d.scratch.data_ptr() + d.need - 64)]
    for kw in bad:
        assert d.call(L, **kw) == EINVAL, kw
        assert b"dlesm_release_f64" in L.dlesm_last_error(), kw
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(d.tensors(), before))
    assert d.call(L) == 0, L.dlesm_last_error()                                         # and the call that is left is fine
    torch.cuda.synchronize()
    d.check(RC.run(c), "after the refusals")


def test_the_python_wrapper(T):
    """psy.particle_release on the one-rank 23 x 19 grid of the particle steps' wrapper tests, against the restatement on the
    grid's own mask; it raises on a dropped particle and returns the record otherwise"""
    torch, D, L = T
    import os
    import drifter_cases as DC
    os.environ["DL_ESM_ALIGNMENT"] = "2"
    try:
        g = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
        g.decompose(23, 19)
        it = g.subdomain.internal
        D.grid_init(g, 1000.0, 1000.0, tmask=DC.mask()[:it.ystop + 1, :it.xstop + 1])
    finally:
        os.environ.pop("DL_ESM_ALIGNMENT", None)
    un = D.r2d_field(g, D.GO_U_POINTS)
    tm = g.tmask_device.cpu().numpy().reshape(g.ny, g.nx)
    box = tuple(D.field_mod.field_bounds(g, D.GO_T_POINTS)[0].box())
    s = g.subdomain
    off = (s.glob.xstart - s.internal.xstart, s.glob.ystart - s.internal.ystart)
    assert off == (-1, -1) and box == (2, 24, 2, 20)          # global cell 1 is the first internal cell
    n = 700
    x, y, rx, ry, first = [6.5, 13.0, 20.0, 30.0], [5.5, 11.0, 17.0, 5.0], [0.0, 8.0, 3.0, 1.0], [0.0, 6.0, 3.0, 1.0], [0, 1000, 2 ** 33, 5]
    src = D.release_sources(x, y, rx, ry, first, count=[5, 100, 64, 9])
    assert src.dtype == torch.int64 and tuple(src.shape) == (4, 8) and src.is_cuda
    host = R.table(x, y, rx, ry, first, [5, 100, 64, 9], tag=np.arange(4))
    assert (src.cpu().numpy() == host).all()
    up = lambda a: torch.from_numpy(a).cuda()
    want = [np.full(n, RC.SENT_F), np.full(n, RC.SENT_F), RC.free_pattern(n, "third"), np.full(n, RC.SENT_I, dtype=np.int64),
            np.full(n, RC.SENT_I, dtype=np.int64), np.full(n, RC.SENT_I, dtype=np.int64)]
    px, py, st, ids, tag, born = (up(a.copy()) for a in want)
    tk = torch.full((1,), 11, dtype=torch.int64, device="cuda")
    rec = D.particle_release(src, px, py, st, ids, un, RC.SEED, tick=4, tick_dev=tk, tag=tag, born=born)
    wrec = R.release_vector(box, off, tm, host, 100, RC.SEED, 15, *want)
    assert isinstance(rec, D._cabi.ReleaseCounts) and bytes(rec) == wrec.tobytes()
    assert rec.released > 50 and rec.foreign > 0 and rec.dropped == 0
    for t, w in zip((px, py, st, ids, tag, born), want):
        assert t.cpu().numpy().tobytes() == w.tobytes()
    assert (src.cpu().numpy() == host).all()
    dev = D.psy.particle_release(src, px, py, st, ids, g, RC.SEED, max_count=50, wait=False)     # clamps, and does not raise
    assert dev.is_cuda and dev.dtype == torch.int32 and dev.numel() == 16
    wrec = R.release_vector(box, off, tm, host, 50, RC.SEED, 0, *want[:4])
    assert (dev.cpu().numpy() == wrec).all() and wrec[R.CLAMPED] == 2 and (st.cpu().numpy() == want[2]).all()
    src[:, R.COUNT] = 200                                                                         # more than the FREE slots are left
    with pytest.raises(D.ReleaseError) as e:
        D.particle_release(src, px, py, st, ids, g, RC.SEED)
    assert e.value.counts.dropped > 0 and e.value.counts.nfree == 0 and isinstance(e.value, D.DlesmError)
    with pytest.raises(D.DlesmError):
        D.particle_release(src, px, py, st, ids.int(), g, RC.SEED)
    with pytest.raises(D.DlesmError):
        D.particle_release(src[:, :7], px, py, st, ids, g, RC.SEED)
    with pytest.raises(D.DlesmError):
        D.particle_release(src, px, py, st, ids, g, RC.SEED, tick=-1)
