"""GPU tests (-m gpu) of the drifters: px, py and status after dlesm_drifter_step_f64 equal both CPU
restatements (tests/drifter_numpy.py) bit for bit on the shared case (tests/drifter_cases.py), on both boxes, for n in {1, 63,
64, 65, 257, 1000, 70001} and nsub in {1, 3}, with an even and an odd leading dimension and bases offset by one element, with
shared input arrays, over twelve successive calls; one call with nsub = 3 is three with nsub = 1; a second stream and repeats
give identical bytes; the slack after element n and every particle that is not ACTIVE are untouched; one capture into a graph
replayed on one stream equals the eager calls; sampling equals numpy for 1, 3 and 8 fields; every refusal returns
DLESM_EINVAL and changes nothing; particles on rows whose element index crosses 2^29 and 2^31 equal the same rows swept as a
small array.  A NaN equals a NaN (the sign of a NaN an operation makes is the machine's); no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import drifter_cases as DC
import drifter_numpy as DN
from particle_gpu import NS, SENT, SLACK, T, _check, _equal, _flow, _particles, _ptr, _up, shared_refusals  # noqa: F401

pytestmark = pytest.mark.gpu


def _step(L, nsub, ld, box, F, n, P, stream=None, h=DC.H, ny=DC.NY):
    return L.dlesm_drifter_step_f64(h, nsub, ld, ny, *box, *[_ptr(t) for t in F], n, *[_ptr(t) for t in P],
                                    C.c_void_p(stream.cuda_stream) if stream is not None else None)


@pytest.mark.parametrize("n", NS)
def test_positions_and_statuses_equal_both_restatements(T, n):
    torch, D, L = T
    idle = DC.particles()[2][:n] != DN.ACTIVE
    x0, y0 = DC.particles()[0][:n], DC.particles()[1][:n]
    for box in DC.BOXES:
        for nsub in (1, 3):
            for ld, off in ((26, 0), (27, 1)):
                F = _flow(torch, ld, off)
                P = _particles(torch, n, off)
                assert _step(L, nsub, ld, box, F, n, P) == 0, L.dlesm_last_error()
                torch.cuda.synchronize()
                got = _check(P, n, DC.reference(box, nsub), (box, nsub, ld, off))
                m = min(n, DC.NSCALAR)
                sx, sy, ss, _ = DC.scalar_reference(box, nsub)
                assert DN.same(got[0][:m], sx[:m]) and DN.same(got[1][:m], sy[:m]) and (got[2][:m] == ss[:m]).all()
                assert DN.same(got[0][:n][idle], x0[idle]) and DN.same(got[1][:n][idle], y0[idle])
    if n == NS[-1]:
        st = DC.reference(DC.BOXES[0], 3)[2]
        assert all((st == s).sum() > 100 for s in range(4))


def test_inputs_are_left_alone_and_may_share_arrays(T):
    torch, D, L = T
    tm, dx_t, dy_t, un, vn = DC.flow()
    F = _flow(torch, 26, 0)
    before = [t.clone() for t in F]
    n = 1000
    for box in DC.BOXES:
        P = _particles(torch, n)
        shared = [F[0], F[1], F[1], F[3], F[3]]                      # dy_t = dx_t, vn = un
        assert _step(L, 2, 26, box, shared, n, P) == 0, L.dlesm_last_error()
        torch.cuda.synchronize()
        want = [a[:n].copy() for a in DC.particles()]
        DN.drifter_step(DC.H, 2, box, tm, dx_t, dx_t, un, un, *want)
        _check(P, n, want, ("shared", box))
        sc = [a[:n].copy() for a in DC.particles()]
        DN.drifter_step_scalar(DC.H, 2, box, tm, dx_t, dx_t, un, un, *sc)
        assert DN.same(sc[0], want[0]) and DN.same(sc[1], want[1]) and (sc[2] == want[2]).all()
    for a, b in zip(F, before):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_twelve_successive_calls_and_the_nsub_identity(T):
    torch, D, L = T
    n = 1000
    for box in DC.BOXES:
        F = _flow(torch, 27, 1)
        P = _particles(torch, n, 1)
        for _ in range(12):
            assert _step(L, 1, 27, box, F, n, P) == 0, L.dlesm_last_error()
        torch.cuda.synchronize()
        want = DC.reference(box, 1, calls=12)
        _check(P, n, want, ("twelve", box))
        Q = _particles(torch, n)
        for nsub in (3, 4, 5):
            assert _step(L, nsub, 27, box, F, n, Q) == 0, L.dlesm_last_error()
        torch.cuda.synchronize()
        _check(Q, n, want, ("3 + 4 + 5", box))
        # three calls with nsub = 1 are one call with nsub = 3, on the device as on the host
        A, B = _particles(torch, DC.POOL), _particles(torch, DC.POOL)
        assert _step(L, 3, 27, box, F, DC.POOL, A) == 0
        for _ in range(3):
            assert _step(L, 1, 27, box, F, DC.POOL, B) == 0
        torch.cuda.synchronize()
        assert _equal(torch, A, B)


def test_repeats_a_second_stream_and_a_graph_give_identical_bytes(T):
    torch, D, L = T
    n, box, ld = 70001, DC.BOXES[0], 26
    F = _flow(torch, ld, 0)
    want = DC.reference(box, 3)
    first = _particles(torch, n)
    assert _step(L, 3, ld, box, F, n, first) == 0
    torch.cuda.synchronize()
    _check(first, n, want, "first")
    second = torch.cuda.Stream()
    for stream in (None, second, second):
        P = _particles(torch, n)
        torch.cuda.synchronize()
        assert _step(L, 3, ld, box, F, n, P, stream) == 0
        torch.cuda.synchronize()
        assert _equal(torch, P, first)
    # one capture of two calls (nsub = 1 and 2) on one stream, no branches; replayed once it equals the eager nsub = 3, and
    # replayed again six substeps
    P = _particles(torch, n)
    start = [t.clone() for t in P]
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        rc1 = _step(L, 1, ld, box, F, n, P, s)
        rc2 = _step(L, 2, ld, box, F, n, P, s)
    assert rc1 == 0 and rc2 == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    assert _equal(torch, P, start)                                                 # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert _equal(torch, P, first)
    graph.replay()
    torch.cuda.synchronize()
    _check(P, n, DC.reference(box, 3, calls=2), "graph twice")


@pytest.mark.parametrize("nfields", [1, 3, 8])
def test_sampling_equals_numpy(T, nfields):
    torch, D, L = T
    n = 1000
    px, py, st = (a[:n] for a in DC.particles())
    host = DC.sample_fields(nfields)
    for box in DC.BOXES:
        for ld, off in ((26, 0), (27, 1)):
            Fd = [_up(torch, DC.embed(f, ld, np.nan), off) for f in host]
            P = _particles(torch, n, off)
            before = [t.clone() for t in P]
            out = [_up(torch, np.full(n + SLACK, SENT), off) for _ in host]
            pf = (C.c_void_p * nfields)(*[t.data_ptr() for t in Fd])
            po = (C.c_void_p * nfields)(*[t.data_ptr() for t in out])
            rc = L.dlesm_drifter_sample_f64(ld, DC.NY, *box, n, *[_ptr(t) for t in P], pf, po, nfields, None)
            assert rc == 0, L.dlesm_last_error()
            torch.cuda.synchronize()
            want = [np.full(n + SLACK, SENT) for _ in host]
            DN.drifter_sample(box, px, py, st, host, [w[:n] for w in want])
            for k in range(nfields):
                assert DN.same(out[k].cpu().numpy(), want[k]), (box, ld, k)
            assert (want[0][:n] != SENT).sum() > 300 and (want[0][:n] == SENT).sum() > 100
            assert _equal(torch, P, before)


def test_the_python_wrappers(T):
    """psy.drifter_step and psy.drifter_sample on a one-rank 26 x 22 grid with the case's mask, against the restatement on
    the grid's own mask and metrics"""
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
    un, vn, c = D.r2d_field(g, D.GO_U_POINTS), D.r2d_field(g, D.GO_V_POINTS), D.r2d_field(g, D.GO_T_POINTS)
    _, _, _, hu, hv = DC.flow()
    un.set_data(hu), vn.set_data(hv)
    hc = DC.sample_fields(1)[0]
    c.set_data(hc)
    n = 1000
    px, py, st = (torch.from_numpy(a[:n].copy()).cuda() for a in DC.particles())
    D.psy.drifter_step(DC.H, px, py, st, un, vn, nsub=3)
    D.drifter_step(DC.H, px, py, st, un, vn)
    got = D.drifter_sample(px, py, st, [c])
    torch.cuda.synchronize()
    tm = g.tmask_device.cpu().numpy()
    dx, dy = g.dx_t_device.cpu().numpy(), g.dy_t_device.cpu().numpy()
    box = c.internal.box()
    assert tuple(box) == (2, 24, 2, 20)
    want = [a[:n].copy() for a in DC.particles()]
    DN.drifter_step(DC.H, 3, box, tm, dx, dy, hu, hv, *want)
    DN.drifter_step(DC.H, 1, box, tm, dx, dy, hu, hv, *want)
    assert DN.same(px.cpu().numpy(), want[0]) and DN.same(py.cpu().numpy(), want[1]) and (st.cpu().numpy() == want[2]).all()
    ws = np.full(n, np.nan)
    DN.drifter_sample(box, *want, [hc], [ws])
    assert len(got) == 1 and DN.same(got[0].cpu().numpy(), ws) and 100 < np.isnan(ws).sum() < n - 100
    assert set(want[2].tolist()) >= {0, 1, 2, 3}
    with pytest.raises(D.DlesmError):
        D.psy.drifter_step(DC.H, px.float(), py, st, un, vn)
    with pytest.raises(D.DlesmError):
        D.psy.drifter_step(DC.H, px, py, st, un, vn, nsub=0)


def test_every_refusal_returns_einval_and_changes_nothing(T):
    torch, D, L = T
    EINVAL = D._cabi.EINVAL
    n, ld, box = 257, 26, DC.BOXES[0]
    F = _flow(torch, ld, 0)
    P = _particles(torch, n)
    before = [t.clone() for t in P]
    fb = [t.clone() for t in F]
    assert _step(L, 1, ld, box, F, 0, P) == 0                                      # n == 0: nothing launched
    assert _step(L, 1, ld, (5, 4, 2, 21), F, n, P) == 0 and _step(L, 1, ld, (2, 25, 9, 8), F, n, P) == 0   # an empty box

    def raw(Fp, Pp, n_=n, nsub=1, h=DC.H, b=box, ny=DC.NY, ld_=ld):
        return L.dlesm_drifter_step_f64(h, nsub, ld_, ny, *b, *[C.c_void_p(p) if p else None for p in Fp], n_,
                                        *[C.c_void_p(p) if p else None for p in Pp], None)

    Fp, Pp = [t.data_ptr() for t in F], [t.data_ptr() for t in P]
    shared_refusals(raw, EINVAL, D._cabi.DRIFTER_MAX_SUB, Fp, Pp, n)
    assert b"overlaps" in L.dlesm_last_error()

    # sampling
    host = DC.sample_fields(2)
    Fd = [_up(torch, f) for f in host]
    out = [_up(torch, np.full(n, SENT)) for _ in host]
    ob = [t.clone() for t in out]

    def sample(fields, outs, nf, n_=n, parts=Pp, b=box):
        pf = (C.c_void_p * max(len(fields), 1))(*fields) if fields is not None else None
        po = (C.c_void_p * max(len(outs), 1))(*outs) if outs is not None else None
        return L.dlesm_drifter_sample_f64(ld, DC.NY, *b, n_, *[C.c_void_p(p) if p else None for p in parts], pf, po, nf, None)

    fp, op = [t.data_ptr() for t in Fd], [t.data_ptr() for t in out]
    assert sample(fp, op, 2, n_=0) == 0 and sample(fp, op, 2, b=(5, 4, 2, 21)) == 0
    assert sample(fp, op, 0) == EINVAL and sample(fp * 5, op * 5, 9) == EINVAL
    assert sample(None, op, 2) == EINVAL and sample(fp, None, 2) == EINVAL
    assert sample([fp[0], None], op, 2) == EINVAL and sample(fp, [op[0], None], 2) == EINVAL
    assert sample([fp[0], fp[1] + 4], op, 2) == EINVAL and sample(fp, [op[0] + 4, op[1]], 2) == EINVAL
    assert sample(fp, op, 2, n_=-1) == EINVAL and sample(fp, op, 2, b=(1, 25, 2, 21)) == EINVAL
    assert sample(fp, op, 2, parts=[None, Pp[1], Pp[2]]) == EINVAL and sample(fp, op, 2, parts=[Pp[0], Pp[1], Pp[2] + 2]) == EINVAL
    assert sample(fp, [op[0], op[0]], 2) == EINVAL and sample(fp, [op[0], fp[0]], 2) == EINVAL
    assert sample(fp, [Pp[0], op[1]], 2) == EINVAL and sample(fp, [op[0], Pp[1]], 2) == EINVAL
    assert sample(fp, [op[0], Pp[2]], 2) == EINVAL
    assert sample([fp[0], fp[0]], op, 2) == 0                                        # read-only inputs may share arrays
    torch.cuda.synchronize()
    assert torch.equal(out[0][:n], out[1][:n]) and not torch.equal(out[0], ob[0])
    for a, b_ in zip(P + F, before + fb):
        assert torch.equal(a.view(torch.int32), b_.view(torch.int32))


def test_the_owner_of_the_three_arrays(T):
    torch, D, L = T
    n, box, ld = 1000, DC.BOXES[0], 26
    F = _flow(torch, ld, 0)
    px, py, st = (np.ascontiguousarray(a[:n]) for a in DC.particles())
    h = C.c_void_p()
    assert L.dlesm_drifters_create(n, C.byref(h)) == 0 and h.value
    cnt, dx, dy, ds = C.c_longlong(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.dlesm_drifters_arrays(h, C.byref(cnt), C.byref(dx), C.byref(dy), C.byref(ds)) == 0 and cnt.value == n
    assert dx.value % 8 == 0 and dy.value % 8 == 0 and ds.value % 4 == 0
    got_s = np.full(n, -1, dtype=np.int32)
    assert L.dlesm_drifters_get(h, None, None, got_s.ctypes.data) == 0 and (got_s == 0).all()          # created all ACTIVE
    assert L.dlesm_drifters_put(h, px.ctypes.data, py.ctypes.data, st.ctypes.data) == 0
    rc = L.dlesm_drifter_step_f64(DC.H, 3, ld, DC.NY, *box, *[_ptr(t) for t in F], n, dx, dy, ds, None)
    assert rc == 0, L.dlesm_last_error()
    gx, gy = np.zeros(n), np.zeros(n)
    assert L.dlesm_drifters_get(h, gx.ctypes.data, gy.ctypes.data, got_s.ctypes.data) == 0             # (waits)
    want = DC.reference(box, 3)
    assert DN.same(gx, want[0][:n]) and DN.same(gy, want[1][:n]) and (got_s == want[2][:n]).all()
    assert L.dlesm_drifters_put(h, px.ctypes.data, py.ctypes.data, None) == 0                          # null status: all ACTIVE
    assert L.dlesm_drifters_get(h, None, None, got_s.ctypes.data) == 0 and (got_s == 0).all()
    assert L.dlesm_drifters_destroy(h) == 0
    assert L.dlesm_drifters_create(0, C.byref(h)) == 0 and L.dlesm_drifters_destroy(h) == 0


# ---------------------------------------------------------------------------------------------- beyond 2^31 elements
BIG_LD, BIG_NY = 46464, 46403


def test_particles_beyond_2_31_elements(T):
    """One 46464 x 46403 f64 array serves as un, vn, dx_t and dy_t (read-only inputs may share arrays) beside an int32 mask
    of the same extent, about 26 GB: a constant but for random three-row bands at the start, where the element index crosses
    2^29 (2^31 bytes of the mask) and 2^31, and at the end.  The particles sit in a band's middle row and move less than a
    cell.  The band's values are 1.0 and 2.0, h = 1/8 and the positions start on sixteenths, so that every operation of the
    rule is exact: the particles of a band then equal, bit for bit, the same three rows swept as a small array with the row
    offset taken off y."""
    torch, D, L = T
    free, _ = torch.cuda.mem_get_info()
    if free < 40e9:
        pytest.skip(f"needs 40 GB of free device memory, {free / 1e9:.0f} GB there")
    assert BIG_LD * BIG_NY > 2 ** 31
    g = torch.Generator(device="cuda")
    g.manual_seed(617)
    A = torch.empty((BIG_NY, BIG_LD), dtype=torch.float64, device="cuda")
    M = torch.empty((BIG_NY, BIG_LD), dtype=torch.int32, device="cuda")
    A.fill_(1.0)
    M.fill_(1)
    rows = sorted({0, BIG_NY - 3, (1 << 29) // BIG_LD - 1, (1 << 31) // BIG_LD - 1})
    assert rows[1] * BIG_LD < 2 ** 29 < (rows[1] + 2) * BIG_LD and rows[2] * BIG_LD < 2 ** 31 < (rows[2] + 2) * BIG_LD
    tbl = torch.tensor([-1, 0, 1, 1, 1, 1, 1, 1], dtype=torch.int32, device="cuda")
    for r in rows:
        A[r:r + 3].copy_(1.0 + torch.randint(0, 2, (3, BIG_LD), device="cuda", generator=g).double())
        M[r:r + 3].copy_(tbl[torch.randint(0, 8, (3, BIG_LD), device="cuda", generator=g)])
    n_band, h, nsub = 4096, 0.125, 3
    px, py = [], []
    for r in rows:
        cols = torch.randint(2, BIG_LD - 2, (n_band,), device="cuda", generator=g).double()
        px.append(cols + torch.randint(0, 16, (n_band,), device="cuda", generator=g).double() / 16.0)
        py.append((r + 2) + torch.randint(0, 4, (n_band,), device="cuda", generator=g).double() / 16.0)
    px, py = torch.cat(px), torch.cat(py)
    n = px.numel()
    st = torch.zeros(n, dtype=torch.int32, device="cuda")
    x0, y0 = px.clone(), py.clone()
    box = (2, BIG_LD - 1, 2, BIG_NY - 1)
    a, m = _ptr(A), _ptr(M)
    rc = L.dlesm_drifter_step_f64(h, nsub, BIG_LD, BIG_NY, *box, m, a, a, a, a, n, _ptr(px), _ptr(py), _ptr(st), None)
    assert rc == 0, L.dlesm_last_error()
    torch.cuda.synchronize()
    seen = set()
    for k, r in enumerate(rows):
        sl = slice(k * n_band, (k + 1) * n_band)
        sx, sy, ss = x0[sl].clone(), (y0[sl] - r).clone(), torch.zeros(n_band, dtype=torch.int32, device="cuda")
        As, Ms = A[r:r + 3], M[r:r + 3]                                          # three rows: a small array of its own
        assert As.is_contiguous() and Ms.is_contiguous()
        a, m = _ptr(As), _ptr(Ms)
        rc = L.dlesm_drifter_step_f64(h, nsub, BIG_LD, 3, 2, BIG_LD - 1, 2, 2, m, a, a, a, a, n_band, _ptr(sx), _ptr(sy),
                                      _ptr(ss), None)
        assert rc == 0, L.dlesm_last_error()
        torch.cuda.synchronize()
        assert torch.equal(px[sl], sx) and torch.equal(py[sl], sy + r) and torch.equal(st[sl], ss), r
        assert bool((sy + r - r == sy).all()) and bool((px[sl] != x0[sl]).any()) and bool((py[sl] != y0[sl]).any())
        assert bool((py[sl].floor() == r + 2).all())                              # nobody left the middle row
        seen |= set(ss.cpu().tolist())
        # and the small sweep equals the array restatement on the host
        hx, hy, hs = x0[sl].cpu().numpy(), (y0[sl] - r).cpu().numpy(), np.zeros(n_band, dtype=np.int32)
        Ah, Mh = As.cpu().numpy(), Ms.cpu().numpy()
        DN.drifter_step(h, nsub, (2, BIG_LD - 1, 2, 2), Mh, Ah, Ah, Ah, Ah, hx, hy, hs)
        assert DN.same(sx.cpu().numpy(), hx) and DN.same(sy.cpu().numpy(), hy) and (ss.cpu().numpy() == hs).all(), r
    assert seen == {0, 2, 3}
    del A, M
    torch.cuda.empty_cache()
