"""GPU tests (-m gpu) of the random walk in a varying diffusivity: px, py and status after
dlesm_random_walk_f64 equal the array restatement (tests/random_walk_numpy.py) bit for bit on the shared case
(tests/drifter_cases.py, tests/random_walk_cases.py), on both boxes, for n in {1, 63, 64, 65, 257, 1000, 70001} and nsub in
{1, 3}, with an even and an odd leading dimension and bases offset by one element, without ids and with random int32 ids, under
a seed whose high word is not zero and from tick 2^32 - 2; the slack after element n, every particle that is not ACTIVE and
the inputs are untouched; a constant field gives dlesm_dispersal_step_f64's bytes on the device and a zero field
dlesm_drifter_step_f64's; what kh_t holds on land changes no byte, and a field that breaks the contract on wet cells does what
the restatement does; the device counter, a captured call replayed twice, a second stream and repeats; a set keeps its random
streams through dlesm_particle_sort_set; the Python wrapper with a field and with a tensor; every refusal of the entry's own;
and the well-mixed basin once on the device, judged by the CPU test's statistics.  A NaN equals a NaN; no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import dispersal_cases as PC
import drifter_cases as DC
import drifter_numpy as DN
import random_walk_cases as RC
import random_walk_numpy as RN
from particle_gpu import _DEV, NS, SENT, SLACK, T, _check, _equal, _flow, _ids, _particles, _ptr, _up, shared_refusals  # noqa: F401

pytestmark = pytest.mark.gpu



def _kh(torch, ld, off, field="kh"):
    """kh_t on the device, SENTINEL in the columns beyond the grid; made once"""
    key = ("kh", ld, off, field)
    if key not in _DEV:
        a = RC.kh_field() if field == "kh" else RC.bad_field() if field == "bad" else RC.constant_field(field)
        _DEV[key] = _up(torch, DC.embed(a, ld, SENT), off)
    return _DEV[key]


def _step(L, nsub, ld, box, F, K, n, P, ids=None, tick=RC.TICK, tick_dev=None, stream=None, seed=RC.SEED, h=DC.H, ny=DC.NY):
    return L.dlesm_random_walk_f64(h, nsub, _ptr(K), RC.signed(seed), tick, _ptr(tick_dev), ld, ny, *box, *[_ptr(t) for t in F], n,
                                   _ptr(ids), *[_ptr(t) for t in P],
                                   C.c_void_p(stream.cuda_stream) if stream is not None else None)


@pytest.mark.parametrize("n", NS)
def test_positions_and_statuses_equal_the_restatement(T, n):
    torch, D, L = T
    idle = DC.particles()[2][:n] != DN.ACTIVE
    x0, y0 = DC.particles()[0][:n], DC.particles()[1][:n]
    assert RC.SEED >> 32 != 0 and RC.TICK + 2 == 2 ** 32
    for box in DC.BOXES:
        for nsub in (1, 3):
            for ld, off in ((26, 0), (27, 1)):
                for with_ids in (False, True):
                    F, K = _flow(torch, ld, off), _kh(torch, ld, off)
                    P = _particles(torch, n, off)
                    ids = _ids(torch, off) if with_ids else None
                    assert _step(L, nsub, ld, box, F, K, n, P, ids) == 0, L.dlesm_last_error()
                    torch.cuda.synchronize()
                    what = (box, nsub, ld, off, with_ids)
                    got = _check(P, n, RC.reference(box, nsub, with_ids), what)
                    m = min(n, DC.NSCALAR)
                    sx, sy, ss, _ = RC.scalar_reference(box, nsub, with_ids)
                    assert DN.same(got[0][:m], sx[:m]) and DN.same(got[1][:m], sy[:m]) and (got[2][:m] == ss[:m]).all(), what
                    assert DN.same(got[0][:n][idle], x0[idle]) and DN.same(got[1][:n][idle], y0[idle]), what
    if n == NS[-1]:
        px, py, st, seen = RC.reference(DC.BOXES[0], 3, False)
        assert all((st == s).sum() > 100 for s in range(4)) and all(seen[k] > 100 for k in RN.CENSUS), seen


def test_inputs_are_left_alone(T):
    torch, D, L = T
    n = 1000
    for ld, off in ((26, 0), (27, 1)):
        F, K, ids = _flow(torch, ld, off), _kh(torch, ld, off), _ids(torch, off)
        before = [t.clone() for t in F + [K, ids]]
        for box in DC.BOXES:
            P = _particles(torch, n, off)
            assert _step(L, 3, ld, box, F, K, n, P, ids) == 0, L.dlesm_last_error()
            torch.cuda.synchronize()
            _check(P, n, RC.reference(box, 3, True), ("inputs", box))
        assert _equal(torch, F + [K, ids], before)


def test_a_constant_field_is_the_dispersal_step_and_a_zero_field_the_drifter_step_on_the_device(T):
    torch, D, L = T
    n, ld = DC.POOL, 27
    F = _flow(torch, ld, 1)
    for box in DC.BOXES:
        for nsub in (1, 3):
            A, B = _particles(torch, n, 1), _particles(torch, n)
            assert _step(L, nsub, ld, box, F, _kh(torch, ld, 1, PC.KH), n, A, _ids(torch)) == 0, L.dlesm_last_error()
            rc = L.dlesm_dispersal_step_f64(DC.H, nsub, PC.KH, RC.signed(RC.SEED), RC.TICK, None, ld, DC.NY, *box,
                                            *[_ptr(t) for t in F], n, _ptr(_ids(torch)), *[_ptr(t) for t in B], None)
            assert rc == 0, L.dlesm_last_error()
            torch.cuda.synchronize()
            assert _equal(torch, A, B), (box, nsub)
            _check(A, n, PC.reference(box, nsub, True), ("constant", box, nsub))
            A, B = _particles(torch, n, 1), _particles(torch, n)
            assert _step(L, nsub, ld, box, F, _kh(torch, ld, 1, 0.0), n, A, _ids(torch)) == 0, L.dlesm_last_error()
            rc = L.dlesm_drifter_step_f64(DC.H, nsub, ld, DC.NY, *box, *[_ptr(t) for t in F], n, *[_ptr(t) for t in B], None)
            assert rc == 0, L.dlesm_last_error()
            torch.cuda.synchronize()
            assert _equal(torch, A, B), (box, nsub)
            _check(A, n, DC.reference(box, nsub), ("zero", box, nsub))


def test_land_values_change_nothing_and_a_field_outside_the_contract_does_what_the_restatement_does(T):
    torch, D, L = T
    n, ld, box = DC.POOL, 26, DC.BOXES[0]
    F = _flow(torch, ld, 0)
    land = DC.mask() == 0
    for fill in (0.0, -5.0, np.inf, 1e300):
        kh = RC.kh_field().copy()
        kh[land] = fill
        P = _particles(torch, n)
        assert _step(L, 3, ld, box, F, _up(torch, kh), n, P, _ids(torch)) == 0, L.dlesm_last_error()
        torch.cuda.synchronize()
        _check(P, n, RC.reference(box, 3, True), ("land", fill))
    P = _particles(torch, n)
    assert _step(L, 3, ld, box, F, _kh(torch, ld, 0, "bad"), n, P, _ids(torch)) == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    _check(P, n, RC.reference(box, 3, True, "bad"), "bad")


def test_the_nsub_identity_with_ticks(T):
    torch, D, L = T
    n, ld = DC.POOL, 26
    F, K = _flow(torch, ld, 0), _kh(torch, ld, 0)
    for box in DC.BOXES:
        ids = _ids(torch)
        A, B = _particles(torch, n), _particles(torch, n)
        assert _step(L, 3, ld, box, F, K, n, A, ids) == 0, L.dlesm_last_error()
        for k in range(3):
            assert _step(L, 1, ld, box, F, K, n, B, ids, tick=RC.TICK + k) == 0, L.dlesm_last_error()
        torch.cuda.synchronize()
        assert _equal(torch, A, B), box
        Z = _particles(torch, n)
        for k in range(3):
            assert _step(L, 1, ld, box, F, K, n, Z, ids) == 0
        torch.cuda.synchronize()
        assert not torch.equal(Z[0], A[0])


def test_the_device_counter_and_a_graph(T):
    torch, D, L = T
    n, box, ld, nsub = DC.POOL, DC.BOXES[0], 26, 3
    F, K, ids = _flow(torch, ld, 0), _kh(torch, ld, 0), _ids(torch)
    want1, want2 = RC.reference(box, nsub, True), RC.reference(box, nsub, True, calls=2)
    # ticks advanced by hand
    H = _particles(torch, n)
    assert _step(L, nsub, ld, box, F, K, n, H, ids) == 0 and _step(L, nsub, ld, box, F, K, n, H, ids, tick=RC.TICK + nsub) == 0
    torch.cuda.synchronize()
    _check(H, n, want2, "two calls by hand")
    # the counter on the device
    tk = torch.zeros(1, dtype=torch.int64, device="cuda")
    P = _particles(torch, n)
    assert _step(L, nsub, ld, box, F, K, n, P, ids, tick_dev=tk) == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    _check(P, n, want1, "one call with the counter")
    assert tk.item() == nsub
    assert _step(L, nsub, ld, box, F, K, n, P, ids, tick_dev=tk) == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    assert _equal(torch, P, H) and tk.item() == 2 * nsub
    # n == 0 and an empty box launch nothing: the counter stays
    assert _step(L, nsub, ld, box, F, K, 0, P, ids, tick_dev=tk) == 0
    assert _step(L, nsub, ld, (5, 4, 2, 21), F, K, n, P, ids, tick_dev=tk) == 0
    torch.cuda.synchronize()
    assert tk.item() == 2 * nsub and _equal(torch, P, H)

    # one capture of one call with the counter on one stream (the step and the counter's launch in a row, no branches):
    # replayed twice it equals the two eager calls
    tk.zero_()
    G = _particles(torch, n)
    start = [t.clone() for t in G]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        rc = _step(L, nsub, ld, box, F, K, n, G, ids, tick_dev=tk, stream=s)
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


def test_repeats_and_a_second_stream_give_identical_bytes(T):
    torch, D, L = T
    n, box, ld = DC.POOL, DC.BOXES[0], 26
    F, K = _flow(torch, ld, 0), _kh(torch, ld, 0)
    first = _particles(torch, n)
    assert _step(L, 3, ld, box, F, K, n, first) == 0
    torch.cuda.synchronize()
    _check(first, n, RC.reference(box, 3, False), "first")
    second = torch.cuda.Stream()
    for stream in (None, second, second):
        P = _particles(torch, n)
        torch.cuda.synchronize()
        assert _step(L, 3, ld, box, F, K, n, P, stream=stream) == 0
        torch.cuda.synchronize()
        assert _equal(torch, P, first)


def test_a_set_keeps_its_random_streams_through_a_sort(T):
    torch, D, L = T
    n, box, ld, nsub = 20000, DC.BOXES[1], 26, 2
    F, K = _flow(torch, ld, 0), _kh(torch, ld, 0)
    px, py, st = (np.ascontiguousarray(a[:n]) for a in DC.particles())
    h = C.c_void_p()
    assert L.dlesm_drifters_create(n, C.byref(h)) == 0 and h.value
    try:
        assert L.dlesm_drifters_put(h, px.ctypes.data, py.ctypes.data, st.ctypes.data) == 0

        def step(tick):
            return L.dlesm_random_walk_set(h, DC.H, nsub, _ptr(K), RC.signed(RC.SEED), tick, None, ld, DC.NY, *box,
                                           *[_ptr(t) for t in F], None)

        assert step(RC.TICK) == 0, L.dlesm_last_error()
        assert L.dlesm_particle_sort_set(h, *box, None) == 0, L.dlesm_last_error()
        assert step(RC.TICK + nsub) == 0, L.dlesm_last_error()
        gx, gy, gs = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
        origin, nlive = np.zeros(n, dtype=np.int32), C.c_longlong()
        assert L.dlesm_drifters_get(h, gx.ctypes.data, gy.ctypes.data, gs.ctypes.data) == 0
        assert L.dlesm_particle_set_origin(h, origin.ctypes.data, C.byref(nlive)) == 0
        assert sorted(origin.tolist()) == list(range(n)) and (origin != np.arange(n)).sum() > n // 2
        want = RC.reference(box, nsub, False, calls=2)
        bx, by, bs = np.empty(n), np.empty(n), np.empty(n, dtype=np.int32)
        bx[origin], by[origin], bs[origin] = gx, gy, gs
        assert DN.same(bx, want[0][:n]) and DN.same(by, want[1][:n]) and (bs == want[2][:n]).all()
    finally:
        assert L.dlesm_drifters_destroy(h) == 0
    assert L.dlesm_random_walk_set(None, DC.H, 1, _ptr(K), 7, 0, None, ld, DC.NY, *box, *[_ptr(t) for t in F],
                                   None) == D._cabi.EINVAL


def test_the_python_wrapper_with_a_field_and_with_a_tensor(T):
    """psy.random_walk on the one-rank 26 x 22 grid of the drifters' wrapper test, against the restatement on the grid's own
    mask and metrics"""
    torch, D, L = T
    import os
    os.environ["DL_ESM_ALIGNMENT"] = "2"
    try:
        g = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
        g.decompose(23, 19)
        it = g.subdomain.internal
        D.grid_init(g, 1000.0, 1000.0, tmask=DC.mask()[:it.ystop + 1, :it.xstop + 1])
        g2 = D.grid_type(D.GO_ARAKAWA_C, (D.GO_BC_EXTERNAL, D.GO_BC_EXTERNAL, D.GO_BC_NONE), D.GO_OFFSET_NE)
        g2.decompose(23, 19)
        D.grid_init(g2, 1000.0, 1000.0, tmask=DC.mask()[:it.ystop + 1, :it.xstop + 1])
    finally:
        os.environ.pop("DL_ESM_ALIGNMENT", None)
    assert (g.nx, g.ny) == (DC.LD, DC.NY)
    un, vn, kf = D.r2d_field(g, D.GO_U_POINTS), D.r2d_field(g, D.GO_V_POINTS), D.r2d_field(g, D.GO_T_POINTS)
    _, _, _, hu, hv = DC.flow()
    tm = g.tmask_device.cpu().numpy()
    kh = np.where(tm != 0, np.nan_to_num(RC.kh_field(), nan=33.0), np.nan)      # the field on the grid's own mask
    un.set_data(hu), vn.set_data(hv), kf.set_data(kh)
    kt = torch.from_numpy(kh).cuda()
    n = 1000
    px, py, st = (torch.from_numpy(a[:n].copy()).cuda() for a in DC.particles())
    ids = torch.from_numpy(RC.ids()[:n].copy()).cuda()
    tk = torch.zeros(1, dtype=torch.int64, device="cuda")
    D.psy.random_walk(DC.H, kf, RC.SEED, RC.TICK, px, py, st, un, vn, nsub=3, ids=ids)
    D.random_walk(DC.H, kt, RC.signed(RC.SEED), 5, px, py, st, un, vn, tick_dev=tk)
    torch.cuda.synchronize()
    assert tk.item() == 1
    dx, dy = g.dx_t_device.cpu().numpy(), g.dy_t_device.cpu().numpy()
    box = D.field_mod.field_bounds(g, D.GO_T_POINTS)[0].box()
    assert tuple(box) == (2, 24, 2, 20)
    want = [a[:n].copy() for a in DC.particles()]
    RN.random_walk(DC.H, 3, kh, RC.SEED, RC.TICK, box, tm, dx, dy, hu, hv, *want, RC.ids()[:n])
    RN.random_walk(DC.H, 1, kh, RC.SEED, 5, box, tm, dx, dy, hu, hv, *want)
    assert DN.same(px.cpu().numpy(), want[0]) and DN.same(py.cpu().numpy(), want[1]) and (st.cpu().numpy() == want[2]).all()
    assert set(want[2].tolist()) >= {0, 1, 2, 3}
    before = [t.clone() for t in (px, py, st)]
    other_t, other_u = D.r2d_field(g2, D.GO_T_POINTS), D.r2d_field(g, D.GO_U_POINTS)
    for bad in (other_t, other_u, kt.float(), kt[:-1], kt.t(), kt.cpu()):
        with pytest.raises(D.DlesmError):
            D.psy.random_walk(DC.H, bad, RC.SEED, 0, px, py, st, un, vn)
    with pytest.raises(D.DlesmError):
        D.psy.random_walk(DC.H, kf, RC.SEED, 0, px.float(), py, st, un, vn)
    with pytest.raises(D.DlesmError):
        D.psy.random_walk(DC.H, kf, RC.SEED, 0, px, py, st, un, vn, nsub=0)
    with pytest.raises(D.DlesmError):
        D.psy.random_walk(DC.H, kf, RC.SEED, 0, px, py, st, un, vn, ids=ids.long())
    with pytest.raises(D.DlesmError):
        D.psy.random_walk(DC.H, kf, RC.SEED, 0, px, py, st, un, vn, tick_dev=tk.int())
    torch.cuda.synchronize()
    assert _equal(torch, (px, py, st), before) and tk.item() == 1


def test_every_refusal_returns_einval_and_changes_nothing(T):
    torch, D, L = T
    EINVAL = D._cabi.EINVAL
    n, ld, box = 257, 26, DC.BOXES[0]
    F = _flow(torch, ld, 0)
    K = _up(torch, RC.kh_field())
    P = _particles(torch, n)
    ids = _up(torch, RC.ids()[:n + SLACK].copy())
    tk = torch.full((2,), 11, dtype=torch.int64, device="cuda")
    before = [t.clone() for t in P + [ids, tk, K]]
    fb = [t.clone() for t in F]
    assert _step(L, 1, ld, box, F, K, 0, P, ids, tick_dev=tk) == 0                   # n == 0: nothing launched
    assert _step(L, 1, ld, (5, 4, 2, 21), F, K, n, P, ids, tick_dev=tk) == 0        # an empty box
    assert _step(L, 1, ld, (2, 25, 9, 8), F, K, n, P, ids, tick_dev=tk) == 0

    def raw(Fp, Pp, n_=n, nsub=1, h=DC.H, b=box, ny=DC.NY, ld_=ld, kh=K.data_ptr(), tick=0, id_=ids.data_ptr(),
            td=tk.data_ptr()):
        return L.dlesm_random_walk_f64(h, nsub, C.c_void_p(kh) if kh else None, 7, tick, C.c_void_p(td) if td else None, ld_, ny,
                                       *b, *[C.c_void_p(p) if p else None for p in Fp], n_,
                                       C.c_void_p(id_) if id_ else None, *[C.c_void_p(p) if p else None for p in Pp], None)

    Fp, Pp = [t.data_ptr() for t in F], [t.data_ptr() for t in P]
    shared_refusals(raw, EINVAL, D._cabi.DRIFTER_MAX_SUB, Fp, Pp, n)
    # the rules of tick, id and tick_dev
    assert raw(Fp, Pp, tick=-1) == EINVAL and raw(Fp, Pp, tick=2 ** 63 - 1) == EINVAL
    assert raw(Fp, Pp, tick=2 ** 63 - 3, nsub=3) == EINVAL
    assert raw(Fp, Pp, id_=ids.data_ptr() + 2) == EINVAL and raw(Fp, Pp, td=tk.data_ptr() + 4) == EINVAL
    for k in range(3):                                                              # id or tick_dev in a particle array
        assert raw(Fp, Pp, id_=Pp[k]) == EINVAL and raw(Fp, Pp, td=Pp[k] + 8) == EINVAL, k
    assert raw(Fp, Pp, id_=Pp[2] - 4 * (n - 1)) == EINVAL                           # the last id is the first status
    for k in range(5):                                                              # tick_dev in an input
        assert raw(Fp, Pp, td=Fp[k] + 8) == EINVAL, k
    assert raw(Fp, Pp, td=ids.data_ptr() + 8) == EINVAL
    # the entry's own
    assert raw(Fp, Pp, kh=None) == EINVAL and b"null kh_t" in L.dlesm_last_error()
    assert raw(Fp, Pp, kh=K.data_ptr() + 4) == EINVAL and b"kh_t is not 8-byte aligned" in L.dlesm_last_error()
    for k in range(3):                                                              # a particle array in kh_t
        Q = list(Pp)
        Q[k] = K.data_ptr() + 8 * (ld * DC.NY) - 8                                  # ... one particle on its last element
        assert raw(Fp, Q, n_=1) == EINVAL and b"overlaps the input kh_t" in L.dlesm_last_error(), (k, L.dlesm_last_error())
        assert raw(Fp, Pp, kh=Pp[k] - 8 * (ld * DC.NY) + 8) == EINVAL, k            # kh_t's last element the array's first
    assert raw(Fp, Pp, td=K.data_ptr()) == EINVAL and raw(Fp, Pp, td=K.data_ptr() + 8 * (ld * DC.NY) - 8) == EINVAL
    assert b"tick_dev overlaps the input kh_t" in L.dlesm_last_error()
    torch.cuda.synchronize()
    for a, b_ in zip(P + [ids, tk, K] + F, before + fb):
        assert torch.equal(a.view(torch.int32), b_.view(torch.int32))
    # and the arguments as they are pass
    assert raw(Fp, Pp, tick=2 ** 63 - 4, nsub=3, td=None) == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    assert not torch.equal(P[0], before[0])


def test_a_well_mixed_cloud_stays_well_mixed_on_the_device(T):
    """the basin, the release, the parameters and the statistics of tests/test_random_walk_numpy.py, the walk by the kernel:
    800 substeps in 8 calls of 100.  The final positions are the restatement's bytes as well (one call of the eight is
    compared, so that the test stays short)."""
    torch, D, L = T
    box, tm, dx, dy, un, vn, kh = RC.basin()
    ld, ny = tm.shape[1], tm.shape[0]
    F = [_up(torch, a) for a in (tm, dx, dy, un, vn)]
    K = _up(torch, kh)
    pool = RC.basin_release()
    P = _particles(torch, RC.WM_N, pool=pool)
    want = [a.copy() for a in pool]
    RN.random_walk(RC.WM_H, RC.WM_SUB, kh, RC.SEED, 0, box, tm, dx, dy, un, vn, *want)
    for c in range(RC.WM_STEPS // RC.WM_SUB):
        assert _step(L, RC.WM_SUB, ld, box, F, K, RC.WM_N, P, tick=c * RC.WM_SUB, h=RC.WM_H, ny=ny) == 0, L.dlesm_last_error()
        if c == 0:
            torch.cuda.synchronize()
            _check(P, RC.WM_N, want, "the first hundred substeps")
    torch.cuda.synchronize()
    px, py, st = (t.cpu().numpy()[:RC.WM_N] for t in P)
    worst = RC.marginal_errors(px, py, st)
    print("largest deviation of a column and of a row count on the device, in standard errors: %.2f %.2f" % worst)
    assert max(worst) < 5.0, worst
