"""GPU tests (-m gpu) of the dispersal step: px, py and status after dlesm_dispersal_step_f64 equal
both CPU restatements (tests/dispersal_numpy.py) bit for bit on the shared case (tests/drifter_cases.py, tests/
dispersal_cases.py), on both boxes, for n in {1, 63, 64, 65, 257, 1000, 70001} and nsub in {1, 3}, with an even and an odd
leading dimension and bases offset by one element, without ids and with random int32 ids (negative ones and duplicates among
them), under a seed whose high word is not zero and from tick 2^32 - 2, which carries into the high counter word; the slack
after element n, every particle that is not ACTIVE and the inputs are untouched; kh = 0 is dlesm_drifter_step_f64; one call
with nsub = 3 is three at successive ticks; the device counter advances by nsub a call and a captured call with it draws
fresh numbers on every replay, one without it the same ones; a second stream and repeats give identical bytes; a set keeps its
particles' random streams through dlesm_particle_sort_set; the Python wrapper; every refusal returns DLESM_EINVAL and changes
nothing.  A NaN equals a NaN (the sign of a NaN an operation makes is the machine's); no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import dispersal_cases as PC
import dispersal_numpy as PN
import drifter_cases as DC
import drifter_numpy as DN
from particle_gpu import NS, SLACK, T, _check, _equal, _flow, _ids, _particles, _ptr, _up, shared_refusals  # noqa: F401

pytestmark = pytest.mark.gpu



def _step(L, nsub, ld, box, F, n, P, ids=None, tick=PC.TICK, tick_dev=None, stream=None, kh=PC.KH, seed=PC.SEED, h=DC.H,
          ny=DC.NY):
    return L.dlesm_dispersal_step_f64(h, nsub, kh, PC.signed(seed), tick, _ptr(tick_dev), ld, ny, *box, *[_ptr(t) for t in F], n,
                                      _ptr(ids), *[_ptr(t) for t in P],
                                      C.c_void_p(stream.cuda_stream) if stream is not None else None)


@pytest.mark.parametrize("n", NS)
def test_positions_and_statuses_equal_both_restatements(T, n):
    torch, D, L = T
    idle = DC.particles()[2][:n] != DN.ACTIVE
    x0, y0 = DC.particles()[0][:n], DC.particles()[1][:n]
    assert PC.SEED >> 32 != 0 and PC.TICK + 2 == 2 ** 32
    for box in DC.BOXES:
        for nsub in (1, 3):
            for ld, off in ((26, 0), (27, 1)):
                for with_ids in (False, True):
                    F = _flow(torch, ld, off)
                    P = _particles(torch, n, off)
                    ids = _ids(torch, off) if with_ids else None
                    assert _step(L, nsub, ld, box, F, n, P, ids) == 0, L.dlesm_last_error()
                    torch.cuda.synchronize()
                    what = (box, nsub, ld, off, with_ids)
                    got = _check(P, n, PC.reference(box, nsub, with_ids), what)
                    m = min(n, DC.NSCALAR)
                    sx, sy, ss, _ = PC.scalar_reference(box, nsub, with_ids)
                    assert DN.same(got[0][:m], sx[:m]) and DN.same(got[1][:m], sy[:m]) and (got[2][:m] == ss[:m]).all(), what
                    assert DN.same(got[0][:n][idle], x0[idle]) and DN.same(got[1][:n][idle], y0[idle]), what
    if n == NS[-1]:
        px, py, st, seen = PC.reference(DC.BOXES[0], 3, False)
        assert all((st == s).sum() > 100 for s in range(4)) and all(v > 100 for v in seen.values()), seen


def test_inputs_are_left_alone(T):
    torch, D, L = T
    n = 1000
    for ld, off in ((26, 0), (27, 1)):
        F, ids = _flow(torch, ld, off), _ids(torch, off)
        before = [t.clone() for t in F + [ids]]
        for box in DC.BOXES:
            P = _particles(torch, n, off)
            assert _step(L, 3, ld, box, F, n, P, ids) == 0, L.dlesm_last_error()
            torch.cuda.synchronize()
            _check(P, n, PC.reference(box, 3, True), ("inputs", box))
        assert _equal(torch, F + [ids], before)


def test_kh_zero_is_the_drifter_step_on_the_device(T):
    torch, D, L = T
    n, ld = DC.POOL, 27
    F = _flow(torch, ld, 1)
    for box in DC.BOXES:
        for nsub in (1, 3):
            A, B = _particles(torch, n, 1), _particles(torch, n)
            assert _step(L, nsub, ld, box, F, n, A, _ids(torch), kh=0.0) == 0, L.dlesm_last_error()
            rc = L.dlesm_drifter_step_f64(DC.H, nsub, ld, DC.NY, *box, *[_ptr(t) for t in F], n, *[_ptr(t) for t in B], None)
            assert rc == 0, L.dlesm_last_error()
            torch.cuda.synchronize()
            assert _equal(torch, A, B), (box, nsub)
            _check(A, n, DC.reference(box, nsub), ("kh = 0", box, nsub))


def test_the_nsub_identity_with_ticks(T):
    torch, D, L = T
    n, ld = DC.POOL, 26
    F = _flow(torch, ld, 0)
    for box in DC.BOXES:
        for with_ids in (False, True):
            ids = _ids(torch) if with_ids else None
            A, B = _particles(torch, n), _particles(torch, n)
            assert _step(L, 3, ld, box, F, n, A, ids) == 0, L.dlesm_last_error()
            for k in range(3):
                assert _step(L, 1, ld, box, F, n, B, ids, tick=PC.TICK + k) == 0, L.dlesm_last_error()
            torch.cuda.synchronize()
            assert _equal(torch, A, B), (box, with_ids)
            # ... and three calls that do not advance the tick are another run
            Z = _particles(torch, n)
            for k in range(3):
                assert _step(L, 1, ld, box, F, n, Z, ids) == 0
            torch.cuda.synchronize()
            assert not torch.equal(Z[0], A[0])


def test_the_device_counter_and_a_graph(T):
    torch, D, L = T
    n, box, ld, nsub = DC.POOL, DC.BOXES[0], 26, 3
    F, ids = _flow(torch, ld, 0), _ids(torch)
    want1, want2 = PC.reference(box, nsub, True), PC.reference(box, nsub, True, calls=2)
    # by hand
    H = _particles(torch, n)
    assert _step(L, nsub, ld, box, F, n, H, ids) == 0 and _step(L, nsub, ld, box, F, n, H, ids, tick=PC.TICK + nsub) == 0
    torch.cuda.synchronize()
    _check(H, n, want2, "two calls by hand")
    # the counter on the device
    tk = torch.zeros(1, dtype=torch.int64, device="cuda")
    P = _particles(torch, n)
    assert _step(L, nsub, ld, box, F, n, P, ids, tick_dev=tk) == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    _check(P, n, want1, "one call with the counter")
    assert tk.item() == nsub
    assert _step(L, nsub, ld, box, F, n, P, ids, tick_dev=tk) == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    assert _equal(torch, P, H) and tk.item() == 2 * nsub
    # n == 0 and an empty box launch nothing: the counter stays
    assert _step(L, nsub, ld, box, F, 0, P, ids, tick_dev=tk) == 0 and _step(L, nsub, ld, (5, 4, 2, 21), F, n, P, ids,
                                                                            tick_dev=tk) == 0
    torch.cuda.synchronize()
    assert tk.item() == 2 * nsub and _equal(torch, P, H)
    # tick and the counter add up: the second call's numbers from tick = TICK - 7 and a counter of nsub + 7
    tk.fill_(nsub + 7)
    Q = _particles(torch, n)
    assert _step(L, nsub, ld, box, F, n, Q, ids) == 0 and _step(L, nsub, ld, box, F, n, Q, ids, tick=PC.TICK - 7, tick_dev=tk) == 0
    torch.cuda.synchronize()
    assert _equal(torch, Q, H) and tk.item() == 2 * nsub + 7

    # one capture of one call with the counter on one stream (the step and the counter's launch in a row, no branches):
    # replayed twice it equals the two eager calls
    tk.zero_()
    G = _particles(torch, n)
    start = [t.clone() for t in G]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        rc = _step(L, nsub, ld, box, F, n, G, ids, tick_dev=tk, stream=s)
    assert rc == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    assert _equal(torch, G, start) and tk.item() == 0                               # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    _check(G, n, want1, "graph once")
    assert tk.item() == nsub
    graph.replay()
    torch.cuda.synchronize()
    assert _equal(torch, G, H) and tk.item() == 2 * nsub
    # the same capture without the counter replays the same kicks: from the same start, the same bytes twice
    graph2 = torch.cuda.CUDAGraph()
    for t, t0 in zip(G, start):
        t.copy_(t0)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph2, stream=s, capture_error_mode="thread_local"):
        rc = _step(L, nsub, ld, box, F, n, G, ids, stream=s)
    assert rc == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    for _ in range(2):
        for t, t0 in zip(G, start):
            t.copy_(t0)
        torch.cuda.synchronize()
        graph2.replay()
        torch.cuda.synchronize()
        _check(G, n, want1, "graph without the counter")


def test_repeats_and_a_second_stream_give_identical_bytes(T):
    torch, D, L = T
    n, box, ld = DC.POOL, DC.BOXES[0], 26
    F = _flow(torch, ld, 0)
    first = _particles(torch, n)
    assert _step(L, 3, ld, box, F, n, first) == 0
    torch.cuda.synchronize()
    _check(first, n, PC.reference(box, 3, False), "first")
    second = torch.cuda.Stream()
    for stream in (None, second, second):
        P = _particles(torch, n)
        torch.cuda.synchronize()
        assert _step(L, 3, ld, box, F, n, P, stream=stream) == 0
        torch.cuda.synchronize()
        assert _equal(torch, P, first)


def test_a_set_keeps_its_random_streams_through_a_sort(T):
    torch, D, L = T
    n, box, ld, nsub = 20000, DC.BOXES[1], 26, 2
    F = _flow(torch, ld, 0)
    px, py, st = (np.ascontiguousarray(a[:n]) for a in DC.particles())
    h = C.c_void_p()
    assert L.dlesm_drifters_create(n, C.byref(h)) == 0 and h.value
    try:
        assert L.dlesm_drifters_put(h, px.ctypes.data, py.ctypes.data, st.ctypes.data) == 0

        def step(tick):
            return L.dlesm_dispersal_step_set(h, DC.H, nsub, PC.KH, PC.signed(PC.SEED), tick, None, ld, DC.NY, *box,
                                              *[_ptr(t) for t in F], None)

        assert step(PC.TICK) == 0, L.dlesm_last_error()
        assert L.dlesm_particle_sort_set(h, *box, None) == 0, L.dlesm_last_error()
        assert step(PC.TICK + nsub) == 0, L.dlesm_last_error()
        gx, gy, gs = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
        origin, nlive = np.zeros(n, dtype=np.int32), C.c_longlong()
        assert L.dlesm_drifters_get(h, gx.ctypes.data, gy.ctypes.data, gs.ctypes.data) == 0
        assert L.dlesm_particle_set_origin(h, origin.ctypes.data, C.byref(nlive)) == 0
        assert sorted(origin.tolist()) == list(range(n)) and (origin != np.arange(n)).sum() > n // 2
        want = PC.reference(box, nsub, False, calls=2)
        bx, by, bs = np.empty(n), np.empty(n), np.empty(n, dtype=np.int32)
        bx[origin], by[origin], bs[origin] = gx, gy, gs
        assert DN.same(bx, want[0][:n]) and DN.same(by, want[1][:n]) and (bs == want[2][:n]).all()
        # a put makes origin the identity again: the slots' numbers are the identities once more
        assert L.dlesm_drifters_put(h, px.ctypes.data, py.ctypes.data, st.ctypes.data) == 0
        assert step(PC.TICK) == 0, L.dlesm_last_error()
        assert L.dlesm_drifters_get(h, gx.ctypes.data, gy.ctypes.data, gs.ctypes.data) == 0
        want = PC.reference(box, nsub, False)
        assert DN.same(gx, want[0][:n]) and DN.same(gy, want[1][:n]) and (gs == want[2][:n]).all()
    finally:
        assert L.dlesm_drifters_destroy(h) == 0


def test_the_python_wrapper(T):
    """psy.dispersal_step on the one-rank 26 x 22 grid of the drifters' wrapper test, against the restatement on the grid's
    own mask and metrics"""
    torch, D, L = T
    import os
    os.environ["DL_ESM_ALIGNMENT"] = "2"
    try:
        g = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
        g.decompose(23, 19)
        it = g.subdomain.internal
        D.grid_init(g, 1000.0, 1000.0, tmask=DC.mask()[:it.ystop + 1, :it.xstop + 1])
    finally:
        os.environ.pop("DL_ESM_ALIGNMENT", None)
    assert (g.nx, g.ny) == (DC.LD, DC.NY)
    un, vn = D.r2d_field(g, D.GO_U_POINTS), D.r2d_field(g, D.GO_V_POINTS)
    _, _, _, hu, hv = DC.flow()
    un.set_data(hu), vn.set_data(hv)
    n = 1000
    px, py, st = (torch.from_numpy(a[:n].copy()).cuda() for a in DC.particles())
    ids = torch.from_numpy(PC.ids()[:n].copy()).cuda()
    tk = torch.zeros(1, dtype=torch.int64, device="cuda")
    D.psy.dispersal_step(DC.H, PC.KH, PC.SEED, PC.TICK, px, py, st, un, vn, nsub=3, ids=ids)
    D.dispersal_step(DC.H, PC.KH, PC.signed(PC.SEED), 5, px, py, st, un, vn, tick_dev=tk)
    torch.cuda.synchronize()
    assert tk.item() == 1
    tm = g.tmask_device.cpu().numpy()
    dx, dy = g.dx_t_device.cpu().numpy(), g.dy_t_device.cpu().numpy()
    box = D.field_mod.field_bounds(g, D.GO_T_POINTS)[0].box()
    assert tuple(box) == (2, 24, 2, 20)
    want = [a[:n].copy() for a in DC.particles()]
    PN.dispersal_step(DC.H, 3, PC.KH, PC.SEED, PC.TICK, box, tm, dx, dy, hu, hv, *want, PC.ids()[:n])
    PN.dispersal_step(DC.H, 1, PC.KH, PC.SEED, 5, box, tm, dx, dy, hu, hv, *want)
    assert DN.same(px.cpu().numpy(), want[0]) and DN.same(py.cpu().numpy(), want[1]) and (st.cpu().numpy() == want[2]).all()
    assert set(want[2].tolist()) >= {0, 1, 2, 3}
    sc = [a[:n].copy() for a in DC.particles()]
    PN.dispersal_step_scalar(DC.H, 3, PC.KH, PC.SEED, PC.TICK, box, tm, dx, dy, hu, hv, *sc, PC.ids()[:n])
    PN.dispersal_step_scalar(DC.H, 1, PC.KH, PC.SEED, 5, box, tm, dx, dy, hu, hv, *sc)
    assert DN.same(sc[0], want[0]) and DN.same(sc[1], want[1]) and (sc[2] == want[2]).all()
    before = [t.clone() for t in (px, py, st)]
    with pytest.raises(D.DlesmError):
        D.psy.dispersal_step(DC.H, PC.KH, PC.SEED, 0, px.float(), py, st, un, vn)
    with pytest.raises(D.DlesmError):
        D.psy.dispersal_step(DC.H, -1.0, PC.SEED, 0, px, py, st, un, vn)
    with pytest.raises(D.DlesmError):
        D.psy.dispersal_step(DC.H, PC.KH, PC.SEED, 0, px, py, st, un, vn, nsub=0)
    with pytest.raises(D.DlesmError):
        D.psy.dispersal_step(DC.H, PC.KH, PC.SEED, 0, px, py, st, un, vn, ids=ids.long())
    with pytest.raises(D.DlesmError):
        D.psy.dispersal_step(DC.H, PC.KH, PC.SEED, 0, px, py, st, un, vn, tick_dev=tk.int())
    torch.cuda.synchronize()
    assert _equal(torch, (px, py, st), before) and tk.item() == 1


def test_every_refusal_returns_einval_and_changes_nothing(T):
    torch, D, L = T
    EINVAL = D._cabi.EINVAL
    n, ld, box = 257, 26, DC.BOXES[0]
    F = _flow(torch, ld, 0)
    P = _particles(torch, n)
    ids = _up(torch, PC.ids()[:n + SLACK].copy())
    tk = torch.full((2,), 11, dtype=torch.int64, device="cuda")
    before = [t.clone() for t in P + [ids, tk]]
    fb = [t.clone() for t in F]
    assert _step(L, 1, ld, box, F, 0, P, ids, tick_dev=tk) == 0                      # n == 0: nothing launched
    assert _step(L, 1, ld, (5, 4, 2, 21), F, n, P, ids, tick_dev=tk) == 0           # an empty box
    assert _step(L, 1, ld, (2, 25, 9, 8), F, n, P, ids, tick_dev=tk) == 0

    def raw(Fp, Pp, n_=n, nsub=1, h=DC.H, b=box, ny=DC.NY, ld_=ld, kh=PC.KH, tick=0, id_=ids.data_ptr(), td=tk.data_ptr()):
        return L.dlesm_dispersal_step_f64(h, nsub, kh, 7, tick, C.c_void_p(td) if td else None, ld_, ny, *b,
                                          *[C.c_void_p(p) if p else None for p in Fp], n_,
                                          C.c_void_p(id_) if id_ else None, *[C.c_void_p(p) if p else None for p in Pp], None)

    Fp, Pp = [t.data_ptr() for t in F], [t.data_ptr() for t in P]
    shared_refusals(raw, EINVAL, D._cabi.DRIFTER_MAX_SUB, Fp, Pp, n)
    # the entry's own
    for kh in (-1.0, -5e-324, float("nan"), float("inf"), float("-inf")):
        assert raw(Fp, Pp, kh=kh) == EINVAL, kh
    assert b"kh" in L.dlesm_last_error()
    assert raw(Fp, Pp, tick=-1) == EINVAL and raw(Fp, Pp, tick=2 ** 63 - 1) == EINVAL
    assert raw(Fp, Pp, tick=2 ** 63 - 3, nsub=3) == EINVAL
    assert raw(Fp, Pp, id_=ids.data_ptr() + 2) == EINVAL and raw(Fp, Pp, td=tk.data_ptr() + 4) == EINVAL
    for k in range(3):                                                              # id or tick_dev in a particle array
        assert raw(Fp, Pp, id_=Pp[k]) == EINVAL and raw(Fp, Pp, id_=Pp[k] + 4 * (n - 1) - (4 * (n - 1)) % 4) == EINVAL, k
        assert raw(Fp, Pp, td=Pp[k] + 8) == EINVAL, k
    assert raw(Fp, Pp, id_=Pp[2] - 4 * (n - 1)) == EINVAL                           # the last id is the first status
    for k in range(5):                                                              # tick_dev in an input
        assert raw(Fp, Pp, td=Fp[k] + 8) == EINVAL, k
    assert raw(Fp, Pp, td=Fp[0] + 4 * (ld * DC.NY) - 8) == EINVAL                   # the mask's last eight bytes
    assert raw(Fp, Pp, td=ids.data_ptr() + 8) == EINVAL
    assert b"overlaps" in L.dlesm_last_error()
    assert L.dlesm_dispersal_step_set(None, DC.H, 1, PC.KH, 7, 0, None, ld, DC.NY, *box, *[_ptr(t) for t in F], None) == EINVAL
    torch.cuda.synchronize()
    for a, b_ in zip(P + [ids, tk] + F, before + fb):
        assert torch.equal(a.view(torch.int32), b_.view(torch.int32))
    # and the arguments as they are pass
    assert raw(Fp, Pp, tick=2 ** 63 - 4, nsub=3, td=None) == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    assert not torch.equal(P[0], before[0])
