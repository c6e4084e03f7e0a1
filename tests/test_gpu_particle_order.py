"""GPU tests (-m gpu) of the particle order: perm and nlive after dlesm_particle_order_f64 equal the
restatement (tests/particle_order_numpy.py: the key rule and numpy's stable argsort) exactly, on every shared case
(tests/particle_order_cases.py: thirteen counts, eight boxes of zero to four radix passes, nine distributions, among them all
particles in one cell, two alternating cells, sorted, reverse sorted, all dead, junk statuses and positions that are not
finite); the words after perm[n) and after the stated scratch bytes are untouched and the inputs unchanged; two runs and a
second stream give identical bytes; dlesm_particle_permute gathers eight arrays of mixed element sizes and skips an index
out of range; sorting commutes with dlesm_drifter_step_f64 bit for bit and stepping only the first nlive changes nothing else;
the order and the gather captured into one linear graph and replayed on changed positions equal the restatement; the
owner's sort keeps its pointers, composes origin over two sorts and resets it on put; every refusal returns DLESM_EINVAL and
changes nothing; the Python wrappers.  Everything is an integer or a bit pattern: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import drifter_cases as DC
import drifter_numpy as DN
import particle_order_cases as PC
import particle_order_numpy as PN

pytestmark = pytest.mark.gpu
SLACK = 64            # guard elements behind perm and behind every gathered array
GUARD = 256           # guard bytes behind the stated scratch bytes
PERM_FILL, BYTE_FILL = -9, 0xA5


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
    return C.c_void_p(t.data_ptr())


def _sp(stream):
    return C.c_void_p(stream.cuda_stream) if stream is not None else None


def _need(L, n):
    b = C.c_longlong(-1)
    assert L.dlesm_particle_order_scratch(n, C.byref(b)) == 0 and b.value >= 0
    return b.value


class Buffers:
    """perm with SLACK guard ints behind it, nlive, and the scratch with GUARD guard bytes behind the stated size"""

    def __init__(self, torch, L, n):
        self.n, self.need = n, _need(L, n)
        self.perm = torch.full((n + SLACK,), PERM_FILL, dtype=torch.int32, device="cuda")
        self.nlive = torch.full((2,), PERM_FILL, dtype=torch.int32, device="cuda")
        self.scratch = torch.full((self.need + GUARD,), BYTE_FILL, dtype=torch.uint8, device="cuda")

    def guards_untouched(self):
        return (bool((self.perm[self.n:] == PERM_FILL).all()) and int(self.nlive[1]) == PERM_FILL and
                bool((self.scratch[self.need:] == BYTE_FILL).all()))


def _order(L, box, n, P, B, stream=None, nlive=True):
    return L.dlesm_particle_order_f64(*box, n, _ptr(P[0]), _ptr(P[1]), _ptr(P[2]), _ptr(B.perm), _ptr(B.nlive) if nlive else None,
                                      _ptr(B.scratch), B.need, _sp(stream))


def _up(torch, arrays):
    return [torch.from_numpy(np.array(a)).cuda() for a in arrays]                 # (a copy: the cases are read-only)


@pytest.mark.parametrize("n", PC.NS)
def test_perm_and_nlive_equal_the_restatement(T, n):
    torch, D, L = T
    B = Buffers(torch, L, n)
    for boxname, box in PC.BOXES.items():
        for dist in PC.DISTS:
            host = PC.case(dist, boxname, n)
            P = _up(torch, host)
            B.perm.fill_(PERM_FILL), B.nlive.fill_(PERM_FILL)
            assert _order(L, box, n, P, B) == 0, L.dlesm_last_error()
            torch.cuda.synchronize()
            want, want_live = PC.reference(dist, boxname, n)
            got = B.perm.cpu().numpy()
            assert np.array_equal(got[:n], want), (dist, boxname, int((got[:n] != want).sum()))
            assert int(B.nlive[0]) == want_live, (dist, boxname)
            assert B.guards_untouched(), (dist, boxname)
            for t, h in zip(P, host):                                      # the inputs, bit for bit
                assert np.array_equal(t.cpu().numpy().view(np.int32), h.view(np.int32)), (dist, boxname)


def test_edge_positions_and_a_null_nlive(T):
    torch, D, L = T
    for boxname, box in PC.BOXES.items():
        if boxname == "empty":
            continue
        px, py, st, live = PC.edge_particles(box)
        n = len(px)
        B = Buffers(torch, L, n)
        P = _up(torch, (px, py, st))
        assert _order(L, box, n, P, B) == 0, L.dlesm_last_error()
        torch.cuda.synchronize()
        want, want_live = PN.order(box, px, py, st)
        assert np.array_equal(B.perm.cpu().numpy()[:n], want) and int(B.nlive[0]) == want_live == 4 and B.guards_untouched()
        B.perm.fill_(PERM_FILL), B.nlive.fill_(PERM_FILL)
        assert _order(L, box, n, P, B, nlive=False) == 0                   # nlive == NULL: perm alone
        torch.cuda.synchronize()
        assert np.array_equal(B.perm.cpu().numpy()[:n], want) and int(B.nlive[0]) == PERM_FILL and B.guards_untouched()


def test_no_particles_and_an_empty_box(T):
    torch, D, L = T
    n = 1000
    B = Buffers(torch, L, n)
    P = _up(torch, PC.case("uniform", "16x16", n))
    assert _order(L, PC.BOXES["16x16"], 0, P, B) == 0                      # n == 0: nlive = 0 and nothing else
    torch.cuda.synchronize()
    assert int(B.nlive[0]) == 0 and bool((B.perm == PERM_FILL).all()) and bool((B.scratch == BYTE_FILL).all())
    B.nlive.fill_(PERM_FILL)
    assert _order(L, PC.BOXES["16x16"], 0, P, B, nlive=False) == 0
    for box in ((5, 4, 3, 10), (3, 10, 5, 4), (5, 4, 5, 4)):               # xstop == xstart - 1: empty, accepted
        B.perm.fill_(PERM_FILL), B.nlive.fill_(PERM_FILL)
        assert _order(L, box, n, P, B) == 0, L.dlesm_last_error()
        torch.cuda.synchronize()
        assert np.array_equal(B.perm.cpu().numpy()[:n], np.arange(n)) and int(B.nlive[0]) == 0 and B.guards_untouched()
        assert bool((B.scratch == BYTE_FILL).all())


def test_two_runs_and_a_second_stream_give_identical_perm(T):
    torch, D, L = T
    n = PC.NS[-1]
    second = torch.cuda.Stream()
    for boxname in ("16x16", "256x256", "5000x5000"):
        for dist in ("uniform", "onecell", "mixed"):
            P = _up(torch, PC.case(dist, boxname, n))
            want = PC.reference(dist, boxname, n)[0]
            for stream in (None, None, second, second):
                B = Buffers(torch, L, n)
                torch.cuda.synchronize()
                assert _order(L, PC.BOXES[boxname], n, P, B, stream) == 0
                torch.cuda.synchronize()
                assert np.array_equal(B.perm.cpu().numpy()[:n], want), (dist, boxname)


DTYPES = ["float64", "int32", "float32", "int64", "float64", "int32", "int64", "float32"]


@pytest.mark.parametrize("n", [1, 257, 70001])
def test_permute_gathers_eight_mixed_arrays_and_skips_a_bad_index(T, n):
    torch, D, L = T
    rng = np.random.default_rng(618 + n)
    perm = rng.permutation(n).astype(np.int32)
    if n > 1:
        bad = rng.choice(n, min(n, 40), replace=False)
        perm[bad] = rng.choice(np.array([-1, n, n + 1, 2 ** 31 - 1, -2 ** 31], dtype=np.int64), len(bad)).astype(np.int32)
    for narrays in (1, 3, 8):
        src = [rng.integers(-2 ** 31, 2 ** 31, n).astype(dt) for dt in DTYPES[:narrays]]
        dst = [np.full(n + SLACK, -7, dtype=dt) for dt in DTYPES[:narrays]]
        S, Dd, Pm = _up(torch, src), _up(torch, dst), _up(torch, [perm])[0]
        ps = (C.c_void_p * narrays)(*[t.data_ptr() for t in S])
        pd = (C.c_void_p * narrays)(*[t.data_ptr() for t in Dd])
        eb = (C.c_int * narrays)(*[a.itemsize for a in src])
        assert L.dlesm_particle_permute(n, _ptr(Pm), narrays, ps, pd, eb, None) == 0, L.dlesm_last_error()
        torch.cuda.synchronize()
        for k in range(narrays):
            PN.permute(perm, src[k], dst[k])
            got = Dd[k].cpu().numpy()
            assert np.array_equal(got, dst[k]), (narrays, k)
            assert np.array_equal(S[k].cpu().numpy(), src[k])
        if n > 1:
            assert (dst[0][:n] == -7).sum() >= len(bad) and (dst[0][n:] == -7).all()


def _drifter_flow(torch):
    tm, dx_t, dy_t, un, vn = DC.flow()
    return _up(torch, [tm, dx_t, dy_t, un, vn])


def _step(L, box, F, n, P, nsub=3):
    return L.dlesm_drifter_step_f64(DC.H, nsub, DC.LD, DC.NY, *box, *[_ptr(t) for t in F], n, *[_ptr(t) for t in P], None)


@pytest.mark.parametrize("box", DC.BOXES)
def test_sorting_commutes_with_the_drifter_step(T, box):
    """sort then step == step then the same permutation, positions and statuses bit for bit; stepping the first nlive alone
    gives the same first nlive and leaves everything behind them as it was"""
    torch, D, L = T
    n = DC.POOL
    F = _drifter_flow(torch)
    host = [a.copy() for a in DC.particles()]
    P = _up(torch, host)
    B = Buffers(torch, L, n)
    assert _order(L, box, n, P, B) == 0, L.dlesm_last_error()
    Q = [torch.empty_like(t) for t in P]
    ps, pd = (C.c_void_p * 3)(*[t.data_ptr() for t in P]), (C.c_void_p * 3)(*[t.data_ptr() for t in Q])
    assert L.dlesm_particle_permute(n, _ptr(B.perm), 3, ps, pd, (C.c_int * 3)(8, 8, 4), None) == 0
    R, before = [t.clone() for t in Q], [t.clone() for t in Q]
    assert _step(L, box, F, n, Q) == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    perm, nlive = PN.order(box, *host)
    assert np.array_equal(B.perm.cpu().numpy()[:n], perm) and int(B.nlive[0]) == nlive and 1000 < nlive < n - 1000
    want = DC.reference(box, 3)
    got = [t.cpu().numpy() for t in Q]
    assert DN.same(got[0], want[0][perm]) and DN.same(got[1], want[1][perm]) and np.array_equal(got[2], want[2][perm])
    assert _step(L, box, F, nlive, R) == 0, L.dlesm_last_error()            # n = nlive: the rest is never read
    torch.cuda.synchronize()
    for whole, front, start in zip(Q, R, before):
        k = nlive * whole.element_size() // 4
        whole, front, start = whole.view(torch.int32), front.view(torch.int32), start.view(torch.int32)
        assert torch.equal(front[:k], whole[:k]) and torch.equal(front[k:], start[k:])
    # (the whole step differs behind nlive in one way only: an ACTIVE particle outside the box is marked LEFT there)
    tail = Q[2][nlive:] != before[2][nlive:]
    assert bool((Q[2][nlive:][tail] == DN.LEFT).all()) and bool((before[2][nlive:][tail] == DN.ACTIVE).all())
    assert torch.equal(Q[0][nlive:].view(torch.int32), before[0][nlive:].view(torch.int32))


def test_order_and_permute_in_one_graph_replayed_on_changed_positions(T):
    torch, D, L = T
    n, boxname = 3 * PC.TILE + 517, "256x256"
    box = PC.BOXES[boxname]
    first, second = PC.case("uniform", boxname, n), PC.case("mixed", boxname, n)
    P = _up(torch, first)
    Q = [torch.full((n + SLACK,), -7, dtype=t.dtype, device="cuda") for t in P]
    B = Buffers(torch, L, n)
    ps, pd = (C.c_void_p * 3)(*[t.data_ptr() for t in P]), (C.c_void_p * 3)(*[t.data_ptr() for t in Q])
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        rc1 = _order(L, box, n, P, B, s)
        rc2 = L.dlesm_particle_permute(n, _ptr(B.perm), 3, ps, pd, (C.c_int * 3)(8, 8, 4), _sp(s))
    assert rc1 == 0 and rc2 == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    assert bool((B.perm == PERM_FILL).all()) and bool((Q[2] == -7).all())                           # captured, not run
    for host, dist in ((first, "uniform"), (second, "mixed"), (first, "uniform")):
        for t, h in zip(P, host):
            t.copy_(torch.from_numpy(np.array(h)))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        perm, nlive = PC.reference(dist, boxname, n)
        assert np.array_equal(B.perm.cpu().numpy()[:n], perm) and int(B.nlive[0]) == nlive and B.guards_untouched(), dist
        for t, h in zip(Q, host):
            got = t.cpu().numpy()
            assert np.array_equal(got[:n].view(np.int32), h[perm].view(np.int32)) and (got[n:] == -7).all(), dist


def test_the_owner_sorts_in_place_and_keeps_the_origin(T):
    torch, D, L = T
    n = 5000
    px, py, st = (np.ascontiguousarray(a[:n]) for a in DC.particles())
    h = C.c_void_p()
    assert L.dlesm_drifters_create(n, C.byref(h)) == 0 and h.value
    ptrs = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
    assert L.dlesm_drifters_arrays(h, None, *[C.byref(p) for p in ptrs]) == 0
    assert L.dlesm_drifters_put(h, px.ctypes.data, py.ctypes.data, st.ctypes.data) == 0
    origin, live = np.full(n, -5, dtype=np.int32), C.c_longlong(77)
    assert L.dlesm_particle_set_origin(h, origin.ctypes.data, C.byref(live)) == 0                   # no sort yet
    assert np.array_equal(origin, np.arange(n)) and live.value == -1
    gx, gy, gs = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)

    def sort_and_get(box):
        assert L.dlesm_particle_sort_set(h, *box, None) == 0, L.dlesm_last_error()
        assert L.dlesm_particle_set_origin(h, origin.ctypes.data, C.byref(live)) == 0
        assert L.dlesm_drifters_get(h, gx.ctypes.data, gy.ctypes.data, gs.ctypes.data) == 0
        now = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
        assert L.dlesm_drifters_arrays(h, None, *[C.byref(p) for p in now]) == 0
        assert [p.value for p in now] == [p.value for p in ptrs]                                    # the pointers stay

    sort_and_get(DC.BOXES[0])
    perm1, nlive1 = PN.order(DC.BOXES[0], px, py, st)
    assert np.array_equal(origin, perm1) and live.value == nlive1 and 100 < nlive1 < n - 100
    assert DN.same(gx, px[perm1]) and DN.same(gy, py[perm1]) and np.array_equal(gs, st[perm1])
    sort_and_get(DC.BOXES[1])                                                                       # a second sort composes
    perm2, nlive2 = PN.order(DC.BOXES[1], px[perm1], py[perm1], st[perm1])
    assert np.array_equal(origin, perm1[perm2]) and live.value == nlive2 and nlive2 < nlive1
    assert DN.same(gx, px[origin]) and DN.same(gy, py[origin]) and np.array_equal(gs, st[origin])
    assert L.dlesm_particle_set_origin(h, None, None) == 0
    assert L.dlesm_drifters_put(h, py.ctypes.data, px.ctypes.data, None) == 0                       # put resets the origin
    assert L.dlesm_particle_set_origin(h, origin.ctypes.data, C.byref(live)) == 0
    assert np.array_equal(origin, np.arange(n)) and live.value == -1
    sort_and_get(DC.BOXES[0])
    perm3, nlive3 = PN.order(DC.BOXES[0], py, px, np.zeros(n, dtype=np.int32))
    assert np.array_equal(origin, perm3) and live.value == nlive3 and DN.same(gx, py[perm3]) and (gs == 0).all()
    assert L.dlesm_drifters_destroy(h) == 0
    assert L.dlesm_drifters_create(0, C.byref(h)) == 0 and L.dlesm_particle_sort_set(h, 2, 5, 2, 5, None) == 0
    assert L.dlesm_particle_set_origin(h, None, C.byref(live)) == 0 and live.value == 0
    assert L.dlesm_drifters_destroy(h) == 0


def test_every_refusal_returns_einval_and_changes_nothing(T):
    torch, D, L = T
    EINVAL = D._cabi.EINVAL
    n, box = 1000, PC.BOXES["16x16"]
    host = PC.case("uniform", "16x16", n)
    P = _up(torch, host)
    B = Buffers(torch, L, n)
    p = [t.data_ptr() for t in P]
    perm, nlive, scratch = B.perm.data_ptr(), B.nlive.data_ptr(), B.scratch.data_ptr()

    def raw(b=box, n_=n, px=p[0], py=p[1], st=p[2], pm=perm, nl=nlive, sc=scratch, nb=B.need):
        v = [C.c_void_p(a) if a else None for a in (px, py, st, pm, nl, sc)]
        return L.dlesm_particle_order_f64(*b, n_, *v[:6], nb, None)

    assert raw(px=None) == EINVAL and raw(py=None) == EINVAL and raw(st=None) == EINVAL                  # null pointers
    assert raw(pm=None) == EINVAL and raw(sc=None) == EINVAL
    assert raw(n_=-1) == EINVAL and raw(n_=2 ** 31) == EINVAL                                            # the count
    assert raw(b=(5, 3, 3, 10)) == EINVAL and raw(b=(3, 10, 5, 3)) == EINVAL                             # the box
    assert raw(b=(1, 65536, 1, 65536)) == EINVAL and raw(b=(1, 65535, 1, 65537)) == EINVAL               # 2^32, 2^32 - 1 cells
    assert raw(b=(-2 ** 31, 2 ** 31 - 1, 1, 1)) == EINVAL
    assert raw(nb=B.need - 1) == EINVAL and raw(nb=0) == EINVAL and raw(nb=-1) == EINVAL                 # the scratch
    assert b"dlesm_particle_order_scratch" in L.dlesm_last_error()
    assert raw(px=p[0] + 4) == EINVAL and raw(py=p[1] + 4) == EINVAL and raw(st=p[2] + 2) == EINVAL      # alignment
    assert raw(pm=perm + 2) == EINVAL and raw(nl=nlive + 2) == EINVAL and raw(sc=scratch + 8) == EINVAL
    for inp in p:                                                                                        # overlaps
        assert raw(pm=inp) == EINVAL and raw(nl=inp) == EINVAL and raw(sc=inp) == EINVAL
    assert raw(nl=p[2] + 4 * (n - 1)) == EINVAL and raw(pm=p[0] + 8 * n - 4) == EINVAL
    assert raw(nl=perm) == EINVAL and raw(nl=perm + 4 * (n - 1)) == EINVAL and raw(sc=perm) == EINVAL
    assert raw(nl=scratch + 16) == EINVAL and raw(pm=scratch + B.need - 4) == EINVAL
    assert b"overlap" in L.dlesm_last_error()
    bytes_ = C.c_longlong(-3)
    assert L.dlesm_particle_order_scratch(-1, C.byref(bytes_)) == EINVAL and bytes_.value == -3
    assert L.dlesm_particle_order_scratch(2 ** 31, C.byref(bytes_)) == EINVAL
    assert L.dlesm_particle_order_scratch(n, None) == EINVAL
    assert L.dlesm_particle_order_scratch(2 ** 31 - 1, C.byref(bytes_)) == 0 and bytes_.value > 3 * 4 * (2 ** 31 - 1)

    # the gather
    S = _up(torch, [np.arange(n, dtype=np.float64), np.arange(n, dtype=np.int32)])
    Dd = [torch.full((n,), -7, dtype=t.dtype, device="cuda") for t in S]
    Pm = torch.arange(n, dtype=torch.int32, device="cuda")
    s, d_, pm = [t.data_ptr() for t in S], [t.data_ptr() for t in Dd], Pm.data_ptr()

    def gather(src=s, dst=d_, eb=(8, 4), k=2, n_=n, perm_=pm):
        ps = (C.c_void_p * 8)(*src) if src is not None else None
        pd = (C.c_void_p * 8)(*dst) if dst is not None else None
        pe = (C.c_int * 8)(*eb) if eb is not None else None
        return L.dlesm_particle_permute(n_, C.c_void_p(perm_) if perm_ else None, k, ps, pd, pe, None)

    assert gather(perm_=None) == EINVAL and gather(src=None) == EINVAL and gather(dst=None) == EINVAL and gather(eb=None) == EINVAL
    assert gather(src=[s[0], None]) == EINVAL and gather(dst=[d_[0], None]) == EINVAL
    assert gather(k=0) == EINVAL and gather(k=-1) == EINVAL
    assert gather(src=s * 4, dst=d_ * 4, eb=(8, 4) * 4, k=9) == EINVAL
    assert gather(n_=-1) == EINVAL and gather(n_=2 ** 31) == EINVAL
    assert gather(eb=(8, 2)) == EINVAL and gather(eb=(16, 4)) == EINVAL and gather(eb=(0, 4)) == EINVAL
    assert gather(src=[s[0] + 4, s[1]]) == EINVAL and gather(dst=[d_[0] + 4, d_[1]]) == EINVAL           # alignment
    assert gather(src=[s[0], s[1] + 2]) == EINVAL and gather(perm_=pm + 2) == EINVAL
    assert gather(dst=[pm, d_[1]], eb=(4, 4)) == EINVAL                                                  # dst on perm
    assert gather(dst=[s[0], d_[1]]) == EINVAL and gather(dst=[d_[0], s[1]]) == EINVAL                   # dst on a src
    assert gather(dst=[s[1], d_[1]], eb=(4, 4)) == EINVAL                                                # ... of another array
    assert gather(dst=[d_[0], d_[0]], eb=(8, 4)) == EINVAL and gather(dst=[d_[0], d_[0] + 8 * n - 4]) == EINVAL
    assert b"overlap" in L.dlesm_last_error()
    assert gather(n_=0) == 0
    assert gather(src=[s[0], s[0]], eb=(8, 8), dst=[d_[0], d_[0]], k=1) == 0                             # one array: fine
    assert L.dlesm_particle_sort_set(None, *box, None) == EINVAL and L.dlesm_particle_set_origin(None, None, None) == EINVAL
    torch.cuda.synchronize()
    assert bool((B.perm == PERM_FILL).all()) and bool((B.nlive == PERM_FILL).all()) and bool((B.scratch == BYTE_FILL).all())
    assert bool((Dd[1] == -7).all()) and torch.equal(Dd[0], S[0])
    for t, h in zip(P, host):
        assert np.array_equal(t.cpu().numpy().view(np.int32), h.view(np.int32))


def test_the_python_wrappers(T):
    """psy.particle_order, particle_permute and particle_sort on a one-rank grid, against the restatement over the grid's T
    internal region; ten arrays go through the gather in two launches"""
    torch, D, L = T
    g = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
    g.decompose(200, 150)
    D.grid_init(g, 1000.0, 1000.0)
    un = D.r2d_field(g, D.GO_U_POINTS)
    box = tuple(D.r2d_field(g, D.GO_T_POINTS).internal.box())
    n = 20000
    rng = np.random.default_rng(6180)
    hx, hy = -5.0 + 215.0 * rng.random(n), -5.0 + 165.0 * rng.random(n)
    hs = rng.choice(np.array([0, 0, 0, 1, 2, 3], dtype=np.int32), n)
    want, want_live = PN.order(box, hx, hy, hs)
    assert n // 4 < want_live < n
    px, py, st = _up(torch, (hx, hy, hs))
    perm, nlive = D.particle_order(px, py, st, g)
    assert D.particle_order is D.psy.particle_order and perm.dtype == torch.int32 and nlive.shape == (1,)
    torch.cuda.synchronize()
    assert np.array_equal(perm.cpu().numpy(), want) and int(nlive[0]) == want_live
    mine = torch.empty(n, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    got = D.psy.particle_order(px, py, st, g, perm=mine, stream=s)
    s.synchronize()
    assert got[0] is mine and np.array_equal(mine.cpu().numpy(), want)
    carry_h = [rng.integers(0, 2 ** 31, n).astype(dt) for dt in (DTYPES + ["int32", "float64"])[:7]]
    carry = _up(torch, carry_h)
    out = D.particle_permute(perm, [px, py, st] + carry)
    torch.cuda.synchronize()
    assert len(out) == 10 and np.array_equal(out[0].cpu().numpy(), hx[want])
    assert np.array_equal(out[9].cpu().numpy(), carry_h[6][want])
    perm2, nlive2 = D.particle_sort(px, py, st, un, carry=carry)
    torch.cuda.synchronize()
    assert np.array_equal(perm2.cpu().numpy(), want) and int(nlive2[0]) == want_live
    assert np.array_equal(px.cpu().numpy(), hx[want]) and np.array_equal(py.cpu().numpy(), hy[want])
    assert np.array_equal(st.cpu().numpy(), hs[want])
    for t, h in zip(carry, carry_h):
        assert np.array_equal(t.cpu().numpy(), h[want])
    with pytest.raises(D.DlesmError):
        D.particle_order(px.float(), py, st, g)
    with pytest.raises(D.DlesmError):
        D.particle_permute(perm, [px[:-1]])
    with pytest.raises(D.DlesmError):
        D.particle_permute(perm, [px.to(torch.int16)])
