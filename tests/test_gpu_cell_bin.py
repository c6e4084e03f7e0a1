"""GPU tests (-m gpu) of the cell bin: after dlesm_cell_bin_f64 three outputs -- the count and two
weighted sums whose bits depend on the order of the additions (tests/cell_bin_cases.py) -- equal the restatement
(tests/cell_bin_numpy.py) in every cell of the box, bit for bit, on nine counts, four boxes and the nine distributions of
tests/particle_order_cases.py: a run inside one wave, one ending on slot 63, one starting on slot 64, runs over two and over
many chunks, a ragged last chunk, all dead, the dead directly behind a live run.  The arrays are larger than the box on every
side and hold a NaN sentinel whose bits are checked afterwards, as are guard bytes behind the stated scratch bytes.  SET, ADD
twice onto a field that is not zero, the sum of the counts against the device's nlive, one case on 4096 x 4096 cells, perm =
NULL on sorted arrays, two runs and a second stream, order and bin in one graph replayed on moved particles, the flag for a
reversed set and for a perm with indices out of range, cell offsets beyond 2^31, the owner's entry, the refusals and the
Python wrapper.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import cell_bin_cases as BC
import cell_bin_numpy as BN
import particle_order_cases as PC
import particle_order_numpy as PN

pytestmark = pytest.mark.gpu
PAD = 3                       # cells of the arrays beyond the box, on every side
GUARD = 256                   # guard bytes behind the stated scratch bytes
BYTE_FILL = 0xA5
SENT_I64 = 0x7FF8DEAD0000BEEF                       # the sentinel's bits: a NaN with a payload
FLAG_FILL = -9


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


def _up(torch, arrays):
    return [torch.from_numpy(np.array(a)).cuda() for a in arrays]                 # (a copy: the cases are read-only)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


class Fields:
    """three arrays of ny x ld doubles for a box, each inside an allocation PAD cells larger on every side that holds the
    sentinel; the library sees the inner arrays (cell (1, 1) at row PAD, column PAD of the allocation)"""

    def __init__(self, torch, box, k=3):
        self.torch, self.box, self.k = torch, box, k
        self.ld, self.rows = max(box[1], 1) + 2 * PAD, max(box[3], 1) + 2 * PAD
        self.ny = self.rows - PAD
        self.mem = torch.empty((k, self.rows, self.ld), dtype=torch.float64, device="cuda")
        self.reset()
        first = (PAD * self.ld + PAD) * 8
        self.ptrs = (C.c_void_p * k)(*[self.mem[a].data_ptr() + first for a in range(k)])

    def reset(self):
        self.mem.view(self.torch.int64).fill_(SENT_I64)

    def inside(self):
        """the box's cells, a view of (k, nyb, nxb)"""
        xstart, xstop, ystart, ystop = self.box
        return self.mem[:, PAD + ystart - 1:PAD + max(ystop, ystart - 1), PAD + xstart - 1:PAD + max(xstop, xstart - 1)]

    def outside_untouched(self):
        bits = self.mem.view(self.torch.int64).clone()
        xstart, xstop, ystart, ystop = self.box
        bits[:, PAD + ystart - 1:PAD + max(ystop, ystart - 1), PAD + xstart - 1:PAD + max(xstop, xstart - 1)] = SENT_I64
        return bool((bits == SENT_I64).all())


class Work:
    """perm, nlive and the order's scratch; the flag; the bin's scratch with GUARD guard bytes behind the stated size"""

    def __init__(self, torch, L, n, k=3):
        self.n, self.k = n, k
        b = C.c_longlong(-1)
        assert L.dlesm_particle_order_scratch(n, C.byref(b)) == 0
        self.order_need = b.value
        assert L.dlesm_cell_bin_scratch(n, k, C.byref(b)) == 0 and b.value >= 0 and b.value % 16 == 0
        self.need = b.value
        self.perm = torch.empty(max(n, 1), dtype=torch.int32, device="cuda")
        self.nlive = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.order_scratch = torch.empty(max(self.order_need, 16), dtype=torch.uint8, device="cuda")
        self.flag = torch.full((2,), FLAG_FILL, dtype=torch.int32, device="cuda")
        self.scratch = torch.full((self.need + GUARD,), BYTE_FILL, dtype=torch.uint8, device="cuda")

    def guards_untouched(self):
        return bool((self.scratch[self.need:] == BYTE_FILL).all()) and int(self.flag[1]) == FLAG_FILL


def _order(L, box, n, P, W, stream=None):
    return L.dlesm_particle_order_f64(*box, n, _ptr(P[0]), _ptr(P[1]), _ptr(P[2]), _ptr(W.perm), _ptr(W.nlive),
                                      _ptr(W.order_scratch), W.order_need, _sp(stream))


def _bin(L, mode, alpha, F, n, P, perm, weights, W, stream=None, flag=True):
    k = len(weights)
    pw = (C.c_void_p * k)(*[w.data_ptr() if w is not None else None for w in weights])
    return L.dlesm_cell_bin_f64(mode, alpha, F.ld, F.ny, *F.box, n, _ptr(P[0]), _ptr(P[1]), _ptr(P[2]),
                                _ptr(perm) if perm is not None else None, k, pw, F.ptrs, _ptr(W.flag) if flag else None,
                                _ptr(W.scratch), W.need, _sp(stream))


def _shape(S, box):
    nxb, nyb, _ = PN.cells(box)
    return S.reshape(S.shape[0], nyb, nxb)


@pytest.mark.parametrize("n", BC.NS)
def test_set_and_add_equal_the_restatement(T, n):
    torch, D, L = T
    W = Work(torch, L, n)
    wts = [None] + _up(torch, [BC.weights(n, 1), BC.weights(n, 2)])
    for boxname in BC.BOXNAMES:
        box = PC.BOXES[boxname]
        F = Fields(torch, box)
        start = np.arange(PN.cells(box)[2], dtype=np.float64).reshape(PN.cells(box)[1], PN.cells(box)[0]) * 0.001 + 1.5
        for dist in PC.DISTS:
            P = _up(torch, PC.case(dist, boxname, n))
            S, has = BC.reference(dist, boxname, n)
            want = [np.empty((PN.cells(box)[1], PN.cells(box)[0])) for _ in range(3)]
            F.reset(), W.flag.fill_(FLAG_FILL)
            assert _order(L, box, n, P, W) == 0, L.dlesm_last_error()
            assert _bin(L, BN.SET, 1.0, F, n, P, W.perm, wts, W) == 0, L.dlesm_last_error()
            torch.cuda.synchronize()
            got = F.inside().cpu().numpy()
            assert np.array_equal(_bits(got), _bits(_shape(S, box))), (dist, boxname, "SET")
            assert F.outside_untouched() and W.guards_untouched() and int(W.flag[0]) == 0, (dist, boxname)
            assert got[0].sum() == int(W.nlive[0]) == PC.reference(dist, boxname, n)[1], (dist, boxname)
            # ADD twice onto a field that is not zero; a cell without particles keeps its bits
            for a in range(3):
                want[a][...] = start
            F.inside().copy_(torch.from_numpy(np.stack(want)))
            for _ in range(2):
                assert _bin(L, BN.ADD, 0.375, F, n, P, W.perm, wts, W) == 0, L.dlesm_last_error()
            torch.cuda.synchronize()
            whole = [np.zeros((F.ny, F.ld)) for _ in range(3)]
            for a in range(3):
                whole[a][box[2] - 1:max(box[3], box[2] - 1), box[0] - 1:max(box[1], box[0] - 1)] = start
            BN.apply(box, BN.ADD, 0.375, S, has, whole)
            BN.apply(box, BN.ADD, 0.375, S, has, whole)
            ref = np.stack([w[box[2] - 1:max(box[3], box[2] - 1), box[0] - 1:max(box[1], box[0] - 1)] for w in whole])
            got = F.inside().cpu().numpy()
            assert np.array_equal(_bits(got), _bits(ref)), (dist, boxname, "ADD")
            assert F.outside_untouched() and W.guards_untouched() and int(W.flag[0]) == 0, (dist, boxname)


def test_a_negative_alpha_stores_minus_zero_in_an_empty_cell_and_no_particles_still_fill(T):
    torch, D, L = T
    n, boxname = 257, "15x16"
    box = PC.BOXES[boxname]
    F, W = Fields(torch, box), Work(torch, L, n)
    wts = [None] + _up(torch, [BC.weights(n, 1), BC.weights(n, 2)])
    P = _up(torch, PC.case("uniform", boxname, n))
    S, has = BC.reference("uniform", boxname, n)
    assert _order(L, box, n, P, W) == 0 and _bin(L, BN.SET, -0.75, F, n, P, W.perm, wts, W) == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    got = F.inside().cpu().numpy()
    assert np.array_equal(_bits(got), _bits(-0.75 * _shape(S, box))) and np.signbit(got[0][~has.reshape(got[0].shape)]).all()
    assert F.outside_untouched() and W.guards_untouched()
    F.reset()
    assert _bin(L, BN.SET, 2.0, F, 0, P, None, wts, W) == 0, L.dlesm_last_error()           # n == 0: the box is filled
    torch.cuda.synchronize()
    assert bool((F.inside().view(torch.int64) == 0).all()) and F.outside_untouched() and int(W.flag[0]) == 0
    F.reset(), W.flag.fill_(FLAG_FILL)
    assert _bin(L, BN.ADD, 2.0, F, 0, P, None, wts, W) == 0                                  # ... and ADD touches no out
    torch.cuda.synchronize()
    assert bool((F.mem.view(torch.int64) == SENT_I64).all()) and int(W.flag[0]) == 0


def test_uniform_on_4096_x_4096(T):
    torch, D, L = T
    n, boxname = 70001, "4096x4096"
    box = PC.BOXES[boxname]
    F, W = Fields(torch, box), Work(torch, L, n)
    wts = [None] + _up(torch, [BC.weights(n, 1), BC.weights(n, 2)])
    P = _up(torch, PC.case("uniform", boxname, n))
    S, has = BC.reference("uniform", boxname, n)
    assert _order(L, box, n, P, W) == 0 and _bin(L, BN.SET, 1.0, F, n, P, W.perm, wts, W) == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    got = F.inside().reshape(3, -1)
    at = torch.from_numpy(np.flatnonzero(has)).cuda()
    assert np.array_equal(_bits(got[:, at].cpu().numpy()), _bits(S[:, has]))
    empty = torch.ones(got.shape[1], dtype=torch.bool, device="cuda")
    empty[at] = False
    assert bool((got.view(torch.int64)[:, empty] == 0).all())
    assert F.outside_untouched() and W.guards_untouched() and int(W.flag[0]) == 0
    assert int(got[0].sum()) == int(W.nlive[0]) == PC.reference("uniform", boxname, n)[1]


def test_two_runs_and_a_second_stream_give_the_same_bytes(T):
    torch, D, L = T
    n, boxname = 70001, "256x256"
    box = PC.BOXES[boxname]
    second = torch.cuda.Stream()
    wts = [None] + _up(torch, [BC.weights(n, 1), BC.weights(n, 2)])
    for dist in ("mixed", "onecell"):
        P = _up(torch, PC.case(dist, boxname, n))
        want = _bits(_shape(BC.reference(dist, boxname, n)[0], box))
        for stream in (None, None, second, second):
            F, W = Fields(torch, box), Work(torch, L, n)
            torch.cuda.synchronize()
            assert _order(L, box, n, P, W, stream) == 0 and _bin(L, BN.SET, 1.0, F, n, P, W.perm, wts, W, stream) == 0
            torch.cuda.synchronize()
            assert np.array_equal(_bits(F.inside().cpu().numpy()), want), dist


def test_order_and_bin_in_one_graph_replayed_on_moved_particles(T):
    torch, D, L = T
    n, boxname = 4097, "256x256"
    box = PC.BOXES[boxname]
    first, second = PC.case("uniform", boxname, n), PC.case("twocells", boxname, n)
    P = _up(torch, first)
    F, W = Fields(torch, box), Work(torch, L, n)
    wts = [None] + _up(torch, [BC.weights(n, 1), BC.weights(n, 2)])
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        rc1 = _order(L, box, n, P, W, s)
        rc2 = _bin(L, BN.SET, 1.0, F, n, P, W.perm, wts, W, s)
    assert rc1 == 0 and rc2 == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    assert bool((F.mem.view(torch.int64) == SENT_I64).all()) and int(W.flag[0]) == FLAG_FILL          # captured, not run
    for host, dist in ((first, "uniform"), (second, "twocells"), (first, "uniform")):
        for t, h in zip(P, host):
            t.copy_(torch.from_numpy(np.array(h)))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = _bits(_shape(BC.reference(dist, boxname, n)[0], box))
        assert np.array_equal(_bits(F.inside().cpu().numpy()), want), dist
        assert F.outside_untouched() and W.guards_untouched() and int(W.flag[0]) == 0, dist


def test_the_flag_of_a_bad_order(T):
    """a reversed set with perm == NULL, and a perm with two indices out of range: unordered = 1, and still nothing outside
    the box, the flag and the scratch is written"""
    torch, D, L = T
    wanted = 0
    for n in (257, 4097):
        for boxname in ("15x16", "256x256"):
            box = PC.BOXES[boxname]
            F, W = Fields(torch, box), Work(torch, L, n)
            wts = [None] + _up(torch, [BC.weights(n, 1), BC.weights(n, 2)])
            P = _up(torch, PC.case("reverse", boxname, n))
            assert BN.slot_keys(box, *PC.case("reverse", boxname, n), None)[1] == 1
            for mode in (BN.SET, BN.ADD):
                assert _bin(L, mode, 1.0, F, n, P, None, wts, W) == 0, L.dlesm_last_error()
                torch.cuda.synchronize()
                assert int(W.flag[0]) == 1 and F.outside_untouched() and W.guards_untouched(), (n, boxname, mode)
            perm = PC.reference("reverse", boxname, n)[0].copy()
            perm[5], perm[n - 57] = n, -1
            Pm = _up(torch, [perm])[0]
            F.reset(), W.flag.fill_(FLAG_FILL)
            assert _bin(L, BN.SET, 1.0, F, n, P, Pm, wts, W) == 0, L.dlesm_last_error()
            torch.cuda.synchronize()
            assert int(W.flag[0]) == 1 and F.outside_untouched() and W.guards_untouched(), (n, boxname)
            wanted += 1
            assert _bin(L, BN.SET, 1.0, F, n, P, Pm, wts, W, flag=False) == 0                # unordered == NULL: no flag
            torch.cuda.synchronize()
            assert F.outside_untouched()
    assert wanted == 4


def test_cell_offsets_beyond_2_31(T):
    """a narrow box high up in an array of more than 2^31 doubles, allocated and not initialised: the box and a band
    around it are set and checked"""
    torch, D, L = T
    ld, ny = 46464, 46300
    assert ld * ny > 2 ** 31 + 2 ** 20
    box = (46000, 46015, 46281, 46296)
    assert (box[2] - 1) * ld > 2 ** 31
    nxb, nyb, ncells = PN.cells(box)
    n = 4097
    rng = np.random.default_rng(619)
    px = box[0] - 2.0 + (nxb + 4.0) * rng.random(n)
    py = box[2] - 2.0 + (nyb + 4.0) * rng.random(n)
    st = rng.choice(np.array([0, 0, 0, 1], dtype=np.int32), n)
    w1 = BC.weights(n, 1)
    perm, nlive = PN.order(box, px, py, st)
    S, has, unordered = BN.sums_array(box, px, py, st, perm, [None, w1])
    assert unordered == 0 and 0 < nlive < n
    big = torch.empty((2, ny, ld), dtype=torch.float64, device="cuda")
    band = big[:, box[2] - 1 - PAD:box[3] + PAD, :]
    band.view(torch.int64).fill_(SENT_I64)
    P = _up(torch, (px, py, st))
    W = Work(torch, L, n, k=2)
    wts = [None] + _up(torch, [w1])
    pw = (C.c_void_p * 2)(None, wts[1].data_ptr())
    po = (C.c_void_p * 2)(big[0].data_ptr(), big[1].data_ptr())
    assert _order(L, box, n, P, W) == 0
    assert L.dlesm_cell_bin_f64(BN.SET, 1.0, ld, ny, *box, n, _ptr(P[0]), _ptr(P[1]), _ptr(P[2]), _ptr(W.perm), 2, pw, po,
                                _ptr(W.flag), _ptr(W.scratch), W.need, None) == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    got = band[:, PAD:PAD + nyb, box[0] - 1:box[1]].cpu().numpy()
    assert np.array_equal(_bits(got), _bits(_shape(S, box))) and int(W.flag[0]) == 0 and W.guards_untouched()
    bits = band.view(torch.int64).clone()
    bits[:, PAD:PAD + nyb, box[0] - 1:box[1]] = SENT_I64
    assert bool((bits == SENT_I64).all())


def test_the_owner_counts_without_moving_the_particles(T):
    torch, D, L = T
    n, boxname = 4097, "15x16"
    box = PC.BOXES[boxname]
    px, py, st = PC.case("mixed", boxname, n)
    S, has = BC.reference("mixed", boxname, n)
    h = C.c_void_p()
    assert L.dlesm_drifters_create(n, C.byref(h)) == 0 and h.value
    assert L.dlesm_drifters_put(h, px.ctypes.data, py.ctypes.data, st.ctypes.data) == 0
    F = Fields(torch, box, k=1)
    for _ in range(2):                                                             # (the second call allocates nothing)
        F.reset()
        assert L.dlesm_cell_bin_set(h, BN.SET, 1.0, F.ld, F.ny, *box, F.ptrs[0], None) == 0, L.dlesm_last_error()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(F.inside().cpu().numpy()[0]), _bits(_shape(S, box)[0])) and F.outside_untouched()
    assert L.dlesm_cell_bin_set(h, BN.ADD, 0.5, F.ld, F.ny, *box, F.ptrs[0], None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(F.inside().cpu().numpy()[0]), _bits(1.5 * _shape(S, box)[0])) and F.outside_untouched()
    gx, gy, gs = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
    assert L.dlesm_drifters_get(h, gx.ctypes.data, gy.ctypes.data, gs.ctypes.data) == 0
    assert np.array_equal(_bits(gx), _bits(px)) and np.array_equal(_bits(gy), _bits(py)) and np.array_equal(gs, st)
    EINVAL = D._cabi.EINVAL
    assert L.dlesm_cell_bin_set(None, BN.SET, 1.0, F.ld, F.ny, *box, F.ptrs[0], None) == EINVAL
    assert L.dlesm_cell_bin_set(h, 2, 1.0, F.ld, F.ny, *box, F.ptrs[0], None) == EINVAL
    assert L.dlesm_cell_bin_set(h, BN.SET, float("inf"), F.ld, F.ny, *box, F.ptrs[0], None) == EINVAL
    assert L.dlesm_cell_bin_set(h, BN.SET, 1.0, F.ld, F.ny, *box, None, None) == EINVAL
    assert L.dlesm_cell_bin_set(h, BN.SET, 1.0, box[1] - 1, F.ny, *box, F.ptrs[0], None) == EINVAL
    assert L.dlesm_drifters_destroy(h) == 0
    assert L.dlesm_drifters_create(0, C.byref(h)) == 0                             # no particles: SET still fills
    F.reset()
    assert L.dlesm_cell_bin_set(h, BN.SET, 1.0, F.ld, F.ny, *box, F.ptrs[0], None) == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    assert bool((F.inside().view(torch.int64) == 0).all()) and F.outside_untouched()
    assert L.dlesm_drifters_destroy(h) == 0


def test_every_refusal_returns_einval_and_changes_nothing(T):
    torch, D, L = T
    EINVAL = D._cabi.EINVAL
    n, boxname = 1000, "15x16"
    box = PC.BOXES[boxname]
    F, W = Fields(torch, box), Work(torch, L, n)
    P = _up(torch, PC.case("sorted", boxname, n))
    wts = _up(torch, [BC.weights(n, 1), BC.weights(n, 2)])
    p = [t.data_ptr() for t in P]
    o = [F.ptrs[a] for a in range(3)]
    fb = F.ld * F.ny * 8

    def raw(mode=BN.SET, alpha=1.0, ld=F.ld, ny=F.ny, b=box, n_=n, px=p[0], py=p[1], st=p[2], pm=None, k=3,
            w=(None, wts[0].data_ptr(), wts[1].data_ptr()), out=tuple(o), fl=W.flag.data_ptr(), sc=W.scratch.data_ptr(),
            nb=W.need):
        pw = (C.c_void_p * 8)(*w) if w is not None else None
        po = (C.c_void_p * 8)(*out) if out is not None else None
        v = [C.c_void_p(a) if a else None for a in (px, py, st, pm)]
        return L.dlesm_cell_bin_f64(mode, alpha, ld, ny, *b, n_, *v, k, pw, po, C.c_void_p(fl) if fl else None,
                                    C.c_void_p(sc) if sc else None, nb, None)

    assert raw(px=None) == EINVAL and raw(py=None) == EINVAL and raw(st=None) == EINVAL              # null pointers
    assert raw(w=None) == EINVAL and raw(out=None) == EINVAL and raw(sc=None) == EINVAL
    assert raw(out=(o[0], None, o[2])) == EINVAL
    assert raw(mode=2) == EINVAL and raw(mode=-1) == EINVAL                                          # the mode, alpha
    assert raw(alpha=float("nan")) == EINVAL and raw(alpha=float("inf")) == EINVAL and raw(mode=BN.ADD, alpha=-float("inf")) == EINVAL
    assert raw(n_=-1) == EINVAL and raw(n_=2 ** 31) == EINVAL                                        # the count
    assert raw(k=0) == EINVAL and raw(k=9) == EINVAL and raw(k=-1) == EINVAL
    assert raw(b=(5, 3, 3, 10)) == EINVAL and raw(b=(3, 10, 5, 3)) == EINVAL                         # the box
    assert raw(b=(0, 5, 1, 5)) == EINVAL and raw(b=(1, F.ld + 1, 1, 5)) == EINVAL and raw(b=(1, 5, 1, F.ny + 1)) == EINVAL
    assert raw(ld=0) == EINVAL and raw(ny=0) == EINVAL
    assert raw(ld=65536, ny=65536, b=(1, 65536, 1, 65536)) == EINVAL                                 # 2^32 cells
    assert raw(nb=W.need - 1) == EINVAL and raw(nb=0) == EINVAL and raw(nb=-1) == EINVAL             # the scratch
    assert b"dlesm_cell_bin_scratch" in L.dlesm_last_error()
    assert raw(px=p[0] + 4) == EINVAL and raw(py=p[1] + 4) == EINVAL and raw(st=p[2] + 2) == EINVAL  # alignment
    assert raw(pm=W.perm.data_ptr() + 2) == EINVAL and raw(fl=W.flag.data_ptr() + 2) == EINVAL
    assert raw(sc=W.scratch.data_ptr() + 8) == EINVAL and raw(out=(o[0] + 4, o[1], o[2])) == EINVAL
    assert raw(w=(None, wts[0].data_ptr() + 4, None)) == EINVAL
    for inp in p + [wts[0].data_ptr()]:                                                              # overlaps
        assert raw(out=(o[0], inp, o[2])) == EINVAL and raw(fl=inp) == EINVAL and raw(sc=inp) == EINVAL
    assert raw(pm=o[1]) == EINVAL and raw(pm=W.scratch.data_ptr()) == EINVAL
    assert raw(out=(o[0], o[0], o[2])) == EINVAL and raw(out=(o[0], o[0] + fb - 8, o[2])) == EINVAL
    assert raw(fl=o[2] + 16) == EINVAL and raw(sc=o[1]) == EINVAL and raw(fl=W.scratch.data_ptr() + 16) == EINVAL
    assert b"overlap" in L.dlesm_last_error()
    bytes_ = C.c_longlong(-3)
    assert L.dlesm_cell_bin_scratch(-1, 1, C.byref(bytes_)) == EINVAL and bytes_.value == -3
    assert L.dlesm_cell_bin_scratch(n, 0, C.byref(bytes_)) == EINVAL and L.dlesm_cell_bin_scratch(n, 9, C.byref(bytes_)) == EINVAL
    assert L.dlesm_cell_bin_scratch(n, 1, None) == EINVAL
    torch.cuda.synchronize()
    assert bool((F.mem.view(torch.int64) == SENT_I64).all()) and bool((W.flag == FLAG_FILL).all())
    assert bool((W.scratch == BYTE_FILL).all())
    assert raw() == 0, L.dlesm_last_error()                                                          # and the call itself is fine
    torch.cuda.synchronize()
    assert int(W.flag[0]) == 0


def test_the_python_wrapper_and_perm_none_on_sorted_arrays(T):
    """psy.cell_bin on a one-rank grid against the restatement over the grid's T internal region; perm = None on arrays that
    psy.particle_sort sorted gives the count of the perm path on the unsorted arrays and, for the sums, the restatement on
    the sorted arrays"""
    torch, D, L = T
    g = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
    g.decompose(200, 150)
    D.grid_init(g, 1000.0, 1000.0)
    un = D.r2d_field(g, D.GO_U_POINTS)
    box = tuple(D.r2d_field(g, D.GO_T_POINTS).internal.box())
    n = 20000
    rng = np.random.default_rng(6190)
    hx, hy = -5.0 + 215.0 * rng.random(n), -5.0 + 165.0 * rng.random(n)
    hs = rng.choice(np.array([0, 0, 0, 1, 2, 3], dtype=np.int32), n)
    w1, w2 = BC.weights(n, 1), BC.weights(n, 2)
    perm, nlive = PN.order(box, hx, hy, hs)
    S, has, _ = BN.sums_array(box, hx, hy, hs, perm, [None, w1, w2])
    px, py, st, d1, d2 = _up(torch, (hx, hy, hs, w1, w2))

    def region(t):
        return t[box[2] - 1:box[3], box[0] - 1:box[1]].cpu().numpy()

    out, flag = D.cell_bin(px, py, st, g, weights=(None, d1, d2))
    assert D.cell_bin is D.psy.cell_bin and len(out) == 3 and out[0].shape == (g.ny, g.nx) and flag.shape == (1,)
    torch.cuda.synchronize()
    assert int(flag[0]) == 0 and int(out[0].sum()) == nlive
    for a in range(3):
        assert np.array_equal(_bits(region(out[a])), _bits(_shape(S, box)[a])), a
        rest = out[a].clone()
        rest[box[2] - 1:box[3], box[0] - 1:box[1]] = 0.0
        assert bool((rest.view(torch.int64) == 0).all())
    count = D.cell_bin(px, py, st, g)[0]                                           # the count alone
    assert len(count) == 1 and torch.equal(count[0], out[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    mine = [torch.full((g.ny, g.nx), 2.0, dtype=torch.float64, device="cuda")]
    got, flag = D.psy.cell_bin(px, py, st, g, weights=[d1], out=mine, perm=torch.from_numpy(perm).cuda(), mode=D._cabi.OUT_ADD,
                               alpha=0.25, stream=s)
    s.synchronize()
    want = np.full(S[1].shape, 2.0)
    want[has] = 2.0 + 0.25 * S[1][has]
    assert got[0] is mine[0] and np.array_equal(_bits(region(mine[0])), _bits(_shape(want[None], box)[0])) and int(flag[0]) == 0
    # sorted in place, weights carried: perm = None is the identity
    D.particle_sort(px, py, st, un, carry=[d1, d2])
    ident = torch.arange(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    S2, _, unordered = BN.sums_array(box, hx[perm], hy[perm], hs[perm], None, [None, w1[perm], w2[perm]])
    assert unordered == 0 and BN.same(S2, S)
    need = C.c_longlong()
    assert L.dlesm_cell_bin_scratch(n, 3, C.byref(need)) == 0
    scratch = torch.empty(need.value, dtype=torch.uint8, device="cuda")
    fl = torch.full((1,), FLAG_FILL, dtype=torch.int32, device="cuda")
    for pm in (None, ident):
        outs = [torch.full((g.ny, g.nx), -1.0, dtype=torch.float64, device="cuda") for _ in range(3)]
        it = box
        rc = L.dlesm_cell_bin_f64(BN.SET, 1.0, g.nx, g.ny, *it, n, _ptr(px), _ptr(py), _ptr(st), _ptr(pm) if pm is not None else None,
                                  3, (C.c_void_p * 3)(None, d1.data_ptr(), d2.data_ptr()),
                                  (C.c_void_p * 3)(*[t.data_ptr() for t in outs]), _ptr(fl), _ptr(scratch), need.value, None)
        assert rc == 0, L.dlesm_last_error()
        torch.cuda.synchronize()
        assert int(fl[0]) == 0
        assert torch.equal(outs[0][box[2] - 1:box[3], box[0] - 1:box[1]], out[0][box[2] - 1:box[3], box[0] - 1:box[1]])
        for a in range(3):
            assert np.array_equal(_bits(region(outs[a])), _bits(_shape(S2, box)[a])), a
    with pytest.raises(D.DlesmError):
        D.cell_bin(px.float(), py, st, g)
    with pytest.raises(D.DlesmError):
        D.cell_bin(px, py, st, g, weights=(d1[:-1],))
    with pytest.raises(D.DlesmError):
        D.cell_bin(px, py, st, g, weights=())
    with pytest.raises(D.DlesmError):
        D.cell_bin(px, py, st, g, out=[torch.zeros(3, dtype=torch.float64, device="cuda")])
