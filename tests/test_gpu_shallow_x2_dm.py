"""GPU test (-m gpu): two shallow-water steps per call on a decomposed grid (dlesm_shallow_step_x2_dm and
dlesm_shallow_step_smooth_x2_dm) in loop-back on one GPU -- rank 0 is its own eight neighbours through depth-2 tables --
against the oracle's step + depth-2 exchange, twice, bit for bit: level n+2 with all its depth-2 halos, level n+1 on the box
grown by one cell (the plain form), the filtered level n+1 with its halos (the filtered form).  Transports: the RCCL group and
the mailboxes with the RCCL group switched off underneath."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
import sw_numpy

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

NAMES = ["u", "v", "p", "uold", "vold", "pold", "unew", "vnew", "pnew", "unew2", "vnew2", "pnew2"]
ALPHA = 0.1


@pytest.fixture(scope="module")
def D():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    import dl_esm_inf_amd as d
    torch.cuda.set_device(0)
    d.parallel_init(0, 1, use_rccl=True)
    return d


class Setup:
    """a halo_width-2 grid, its twelve fields and a loop-back plan of depth `depth`"""

    def __init__(self, D, nx, ny, alignment, peer, depth=2, halo_width=2):
        from dm_overhead import loopback_tables
        self.D, self.L = D, D._cabi.lib()
        if alignment is None:
            os.environ.pop("DL_ESM_ALIGNMENT", None)
        else:
            os.environ["DL_ESM_ALIGNMENT"] = str(alignment)
        g = D.grid_type(D.GO_ARAKAWA_C, (1, 1, 2), D.GO_OFFSET_NE)
        g.decompose(nx, ny, halo_width=halo_width)
        D.grid_init(g, 1.0, 1.0)
        os.environ.pop("DL_ESM_ALIGNMENT", None)
        pts = {"u": D.GO_U_POINTS, "v": D.GO_V_POINTS, "p": D.GO_T_POINTS}
        self.g = g
        self.F = {n: D.r2d_field(g, pts[n[0]]) for n in NAMES}
        self.it = self.F["p"].internal
        self.t = loopback_tables(D, self.it, depth)
        self.plan = C.c_void_p()
        D._cabi.check(self.L.dlesm_halo_plan_create(C.byref(self.t), g.nx, g.ny, C.byref(self.plan)))
        g._halo_plan = self.plan
        self.peer = peer
        if peer:
            D.psy.halo_connect_peers(g, 3)
            self.L.dlesm_set_tuning(b"dm_skip_parts", 1)        # no RCCL group: only the mailboxes can move the halos
        self.oc = O.Comms()
        C.memmove(C.byref(self.oc), C.byref(self.t), C.sizeof(self.oc))

    def fill(self, seed):
        """levels n and n-1 hashed, everything else 9.0; both input levels exchanged (depth 2)"""
        import torch
        D, F = self.D, self.F
        for k, n in enumerate(NAMES[:6]):
            D.psy.hash_init(F[n], seed + k)
            F[n].data.mul_(0.01)
            F[n].data.add_(1.0 if n[0] == "p" else -0.005)
        for n in NAMES[6:]:
            D.set_field(F[n], 9.0)
        D.psy.halo_exchange_multi([F["u"], F["v"], F["p"]])
        D.psy.halo_exchange_multi([F["uold"], F["vold"], F["pold"]])
        torch.cuda.synchronize()
        return {n: F[n].get_data() for n in NAMES}

    def xchg(self, arrays):
        for a in arrays:
            assert O.exchange_all([a], [self.g.nx], [self.oc]) == 0

    def close(self):
        self.D._cabi.check(self.L.dlesm_halo_plan_destroy(self.plan))
        self.g._halo_plan = None
        self.L.dlesm_set_tuning(b"dm_skip_parts", 0)
        self.L.dlesm_set_tuning(b"sw_x2_dm_overlap", 0)


def oracle_step(S, prm, cur, old, new):
    """one plain step over the box + depth-2 exchange of the new level"""
    O.sw_step(prm, S.g.nx, S.it.box(), *cur, *old, *new)
    S.xchg(new)


def oracle_smooth_step(S, prm, cur, old, new):
    """one filtered step: step over the box, time_smooth of the old level over the box, depth-2 exchange of both"""
    O.sw_step(prm, S.g.nx, S.it.box(), *cur, *old, *new)
    for c, nw, o in zip(cur, new, old):
        sw_numpy.time_smooth_numpy(ALPHA, S.it.box(), c, nw, o)
    S.xchg(new)
    S.xchg(old)


def grown_mask(S):
    """cells of the box grown by one cell (every side has a neighbour in loop-back)"""
    it = S.it
    m = np.zeros((S.g.ny, S.g.nx), dtype=bool)
    m[it.ystart - 2:it.ystop + 1, it.xstart - 2:it.xstop + 1] = True
    return m


def halo_view(S, a):
    """the box and its depth-2 halos"""
    it = S.it
    return a[it.ystart - 3:it.ystop + 2, it.xstart - 3:it.xstop + 2]


SHAPES = [(2, 2, 2), (3, 5, 2), (5, 4, None), (4, 3, 8), (40, 33, 8), (257, 66, 64), (130, 9, None), (64, 70, 64),
          (700, 300, 64)]


def _diff(got, want):
    return np.argwhere(got != want)[:5]


@pytest.mark.parametrize("peer", [0, 1])
@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("nx,ny,alignment", SHAPES)
def test_x2_dm_one_call(D, nx, ny, alignment, overlap, peer):
    """one call of the plain form against step + depth-2 exchange, twice: unew2.. whole arrays (halos included), unew.. on
    the grown box (elsewhere what they held).  overlap=0: the whole box, then the exchange (sw_x2_dm_overlap = 0)."""
    import torch
    S = Setup(D, nx, ny, alignment, peer)
    try:
        D._cabi.lib().dlesm_set_tuning(b"sw_x2_dm_overlap", overlap)
        H = S.fill(300)
        prm = D.psy.shallow_params(1.0e5, 1.0e5, 90.0)
        W = {n: H[n].copy() for n in NAMES}
        n1 = [W["unew"], W["vnew"], W["pnew"]]
        oracle_step(S, prm, [W["u"], W["v"], W["p"]], [W["uold"], W["vold"], W["pold"]], n1)
        oracle_step(S, prm, n1, [W["u"], W["v"], W["p"]], [W["unew2"], W["vnew2"], W["pnew2"]])
        D.psy.invoke_shallow_step_x2_dm(prm, *[S.F[n] for n in NAMES])
        torch.cuda.synchronize()
        m = grown_mask(S)
        for n in NAMES[9:]:
            got = S.F[n].get_data()
            assert np.array_equal(got, W[n]), (n, _diff(got, W[n]))
        for n in NAMES[6:9]:
            got, want = S.F[n].get_data(), np.where(m, W[n], H[n])
            assert np.array_equal(got, want), (n, _diff(got, want))
        for n in NAMES[:6]:
            assert np.array_equal(S.F[n].get_data(), H[n]), n
    finally:
        S.close()


@pytest.mark.parametrize("peer", [0, 1])
@pytest.mark.parametrize("nx,ny,alignment", [(3, 5, 2), (40, 33, 8), (130, 9, None), (257, 66, 64)])
def test_x2_dm_time_loop(D, nx, ny, alignment, peer):
    """K = 4 calls with the rotation (cur, old, new1, new2) <- (new2, new1, old, cur) against 2K oracle steps"""
    import torch
    S = Setup(D, nx, ny, alignment, peer)
    try:
        H = S.fill(400)
        prm = D.psy.shallow_params(1.0e5, 1.0e5, 90.0)
        tri = lambda a, b, c: [H[a].copy(), H[b].copy(), H[c].copy()]     # noqa: E731
        cur, old = tri("u", "v", "p"), tri("uold", "vold", "pold")
        for _ in range(8):
            new = [np.zeros_like(cur[0]) for _ in range(3)]
            oracle_step(S, prm, cur, old, new)
            cur, old = new, cur
        cur_f = [S.F["u"], S.F["v"], S.F["p"]]
        old_f = [S.F["uold"], S.F["vold"], S.F["pold"]]
        n1_f = [S.F["unew"], S.F["vnew"], S.F["pnew"]]
        n2_f = [S.F["unew2"], S.F["vnew2"], S.F["pnew2"]]
        for _ in range(4):
            D.psy.invoke_shallow_step_x2_dm(prm, *cur_f, *old_f, *n1_f, *n2_f)
            cur_f, old_f, n1_f, n2_f = n2_f, n1_f, old_f, cur_f
        torch.cuda.synchronize()
        m = grown_mask(S)
        for k in range(3):
            got, want = halo_view(S, cur_f[k].get_data()), halo_view(S, cur[k])
            assert np.array_equal(got, want), (k, _diff(got, want))
            got = old_f[k].get_data()
            assert np.array_equal(got[m], old[k][m]), k
    finally:
        S.close()


@pytest.mark.parametrize("peer", [0, 1])
@pytest.mark.parametrize("overlap", [1, 0])
@pytest.mark.parametrize("ncalls", [1, 3])
@pytest.mark.parametrize("nx,ny,alignment", SHAPES)
def test_smooth_x2_dm(D, nx, ny, alignment, ncalls, overlap, peer):
    """ncalls calls of the filtered form, ping-pong (cur, old) <-> (unew2.., uold2..), against 2 x ncalls filtered oracle steps
    (step, time_smooth of the old level over the box, depth-2 exchange of both levels): the newest level and the filtered
    previous one on the box and in their depth-2 halos.  overlap=1: frame strips first, the six-field exchange (two turns
    over the mailboxes) on the side stream behind the interior (sw_x2_dm_overlap = 1)."""
    import torch
    S = Setup(D, nx, ny, alignment, peer)
    try:
        D._cabi.lib().dlesm_set_tuning(b"sw_x2_dm_overlap", overlap)
        H = S.fill(500)
        prm = D.psy.shallow_params(1.0e5, 1.0e5, 90.0)
        cur = [H["u"].copy(), H["v"].copy(), H["p"].copy()]
        old = [H["uold"].copy(), H["vold"].copy(), H["pold"].copy()]
        for _ in range(2 * ncalls):
            new = [np.zeros_like(cur[0]) for _ in range(3)]
            oracle_smooth_step(S, prm, cur, old, new)     # old <- the filtered `cur`, in place
            cur = new
        A = [S.F[n] for n in ("u", "v", "p", "uold", "vold", "pold")]
        B = [S.F[n] for n in ("unew2", "vnew2", "pnew2", "unew", "vnew", "pnew")]
        for _ in range(ncalls):
            D.psy.invoke_shallow_step_smooth_x2_dm(prm, ALPHA, *A, *B)
            A, B = B, A
        torch.cuda.synchronize()
        for k in range(3):
            got = halo_view(S, A[k].get_data())
            want = halo_view(S, cur[k])
            assert np.array_equal(got, want), ("level", k, _diff(got, want))
            got = halo_view(S, A[3 + k].get_data())
            want = halo_view(S, old[k])
            assert np.array_equal(got, want), ("filtered", k, _diff(got, want))
    finally:
        S.close()


@pytest.mark.parametrize("form", ["plain", "smooth"])
def test_x2_dm_8192_tile(D, form):
    """one 8192^2 tile in loop-back (RCCL), whole fields compared"""
    import torch
    S = Setup(D, 8192, 8192, 64, 0)
    try:
        H = S.fill(600)
        prm = D.psy.shallow_params(1.0e5, 1.0e5, 90.0)
        W = {n: H[n].copy() for n in NAMES}
        cur, old = [W["u"], W["v"], W["p"]], [W["uold"], W["vold"], W["pold"]]
        if form == "plain":
            n1 = [W["unew"], W["vnew"], W["pnew"]]
            oracle_step(S, prm, cur, old, n1)
            oracle_step(S, prm, n1, cur, [W["unew2"], W["vnew2"], W["pnew2"]])
            D.psy.invoke_shallow_step_x2_dm(prm, *[S.F[n] for n in NAMES])
            torch.cuda.synchronize()
            for n in NAMES[9:]:
                assert np.array_equal(S.F[n].get_data(), W[n]), n
            m = grown_mask(S)
            for n in NAMES[6:9]:
                assert np.array_equal(S.F[n].get_data(), np.where(m, W[n], H[n])), n
        else:
            n1 = [np.zeros_like(cur[0]) for _ in range(3)]
            oracle_smooth_step(S, prm, cur, old, n1)       # old <- filtered n
            n2 = [np.zeros_like(cur[0]) for _ in range(3)]
            oracle_smooth_step(S, prm, n1, old, n2)        # old <- filtered n+1
            A = [S.F[n] for n in ("u", "v", "p", "uold", "vold", "pold")]
            B = [S.F[n] for n in ("unew2", "vnew2", "pnew2", "unew", "vnew", "pnew")]
            D.psy.invoke_shallow_step_smooth_x2_dm(prm, ALPHA, *A, *B)
            torch.cuda.synchronize()
            for k in range(3):
                assert np.array_equal(halo_view(S, B[k].get_data()), halo_view(S, n2[k])), k
                assert np.array_equal(halo_view(S, B[3 + k].get_data()), halo_view(S, old[k])), k
    finally:
        S.close()


@pytest.mark.parametrize("nx,ny,alignment", [(40, 33, 8), (37, 21, None), (4, 3, 2)])
def test_x2_dm_plan_without_messages(D, nx, ny, alignment):
    """a one-rank grid decomposed with halo_width = 2 has a plan without messages: each distributed entry is its
    single-domain entry, bit for bit, in all twelve fields (the same inputs given to both)"""
    import torch
    if alignment is None:
        os.environ.pop("DL_ESM_ALIGNMENT", None)
    else:
        os.environ["DL_ESM_ALIGNMENT"] = str(alignment)
    g = D.grid_type(D.GO_ARAKAWA_C, (1, 1, 2), D.GO_OFFSET_NE)
    g.decompose(nx, ny, halo_width=2)
    D.grid_init(g, 1.0, 1.0)
    os.environ.pop("DL_ESM_ALIGNMENT", None)
    assert g.comm_tables.nsend == 0 and g.comm_tables.nrecv == 0
    pts = {"u": D.GO_U_POINTS, "v": D.GO_V_POINTS, "p": D.GO_T_POINTS}
    prm = D.psy.shallow_params(1.0e5, 1.0e5, 90.0)
    for form in ("plain", "smooth"):
        A = [D.r2d_field(g, pts[n[0]]) for n in NAMES]
        B = [D.r2d_field(g, pts[n[0]]) for n in NAMES]
        for k, (a, b) in enumerate(zip(A, B)):
            D.psy.hash_init(a, 800 + k)
            a.data.mul_(0.01)
            a.data.add_(1.0 if NAMES[k][0] == "p" else -0.005)
            b.data.copy_(a.data)
        if form == "plain":
            D.psy.invoke_shallow_step_x2_dm(prm, *A)
            D.psy.invoke_shallow_step_x2(prm, *B)
        else:
            D.psy.invoke_shallow_step_smooth_x2_dm(prm, ALPHA, *A)
            D.psy.invoke_shallow_step_smooth_x2(prm, ALPHA, *B)
        torch.cuda.synchronize()
        for n, a, b in zip(NAMES, A, B):
            assert np.array_equal(a.get_data(), b.get_data()), (form, n)


def test_x2_dm_refusals(D):
    """a depth-1 plan, aliased arrays, and a halo_width-1 grid through the Python wrappers are refused"""
    prm = D.psy.shallow_params(1.0e5, 1.0e5, 90.0)
    S = Setup(D, 40, 33, 8, 0, depth=1)
    try:
        S.fill(700)
        with pytest.raises(D._cabi.DlesmError, match="depth"):
            D.psy.invoke_shallow_step_x2_dm(prm, *[S.F[n] for n in NAMES])
        with pytest.raises(D._cabi.DlesmError, match="depth"):
            D.psy.invoke_shallow_step_smooth_x2_dm(prm, ALPHA, *[S.F[n] for n in NAMES])
    finally:
        S.close()
    S = Setup(D, 40, 33, 8, 0)
    try:
        S.fill(701)
        args = [S.F[n] for n in NAMES]
        args[11] = args[3]                   # pnew2 is uold
        with pytest.raises(D._cabi.DlesmError, match="overlap"):
            D.psy.invoke_shallow_step_x2_dm(prm, *args)
        with pytest.raises(D._cabi.DlesmError, match="overlap"):
            D.psy.invoke_shallow_step_smooth_x2_dm(prm, ALPHA, *args)
    finally:
        S.close()
    S = Setup(D, 40, 33, 8, 0, depth=1, halo_width=1)
    try:
        S.fill(702)
        with pytest.raises(D._cabi.DlesmError, match="halo_width"):
            D.psy.invoke_shallow_step_x2_dm(prm, *[S.F[n] for n in NAMES])
        with pytest.raises(D._cabi.DlesmError, match="halo_width"):
            D.psy.invoke_shallow_step_smooth_x2_dm(prm, ALPHA, *[S.F[n] for n in NAMES])
    finally:
        S.close()


@pytest.mark.parametrize("xstop", [128, 129])
def test_both_sides_of_the_lane_fit_on_an_odd_leading_dimension(D, xstop):
    """dlesm_shallow_step_x2_dm on raw 131 x 12 arrays (16-byte aligned bases) with a loop-back depth-2 plan for the box
    (3:xstop, 3:10): with an east neighbour the last computed column is xstop + 1, on either side of the last whole two-column
    chunk of a row (2 * (ld / 2) - 1 = 129): the wave tiles at 128, two single steps at 129.  Level n+2 whole arrays, level
    n+1 on the grown box, inputs untouched, bit for bit the oracle's step + depth-2 exchange, twice."""
    import torch
    from dm_overhead import loopback_tables
    L = D._cabi.lib()
    ld, ny, box = 131, 12, (3, xstop, 3, 10)
    t = loopback_tables(D, D._cabi.Region(xstop - 2, 8, *box), 2)
    oc = O.Comms()
    C.memmove(C.byref(oc), C.byref(t), C.sizeof(oc))
    rng = np.random.default_rng(131 * 12 + xstop)
    H = [rng.random((ny, ld)) * 0.01 + (1.0 if k % 3 == 2 else -0.005) for k in range(6)] + [np.full((ny, ld), 9.0) for _ in range(6)]
    for h in H[:6]:
        assert O.exchange_all([h], [ld], [oc]) == 0
    Dv = [torch.from_numpy(h).cuda() for h in H]
    assert all(d.data_ptr() % 16 == 0 for d in Dv)
    W = [h.copy() for h in H]
    prm = D.psy.shallow_params(1.0e5, 1.0e5, 90.0)
    for cur, old, new in ((W[:3], W[3:6], W[6:9]), (W[6:9], W[:3], W[9:])):
        O.sw_step(prm, ld, box, *cur, *old, *new)
        for a in new:
            assert O.exchange_all([a], [ld], [oc]) == 0
    plan = C.c_void_p()
    D._cabi.check(L.dlesm_halo_plan_create(C.byref(t), ld, ny, C.byref(plan)))
    try:
        D._cabi.check(L.dlesm_shallow_step_x2_dm(plan, C.byref(prm), ld, ny, *box, *[C.c_void_p(d.data_ptr()) for d in Dv], None))
        torch.cuda.synchronize()
        grown = np.zeros((ny, ld), dtype=bool)
        grown[box[2] - 2:box[3] + 1, box[0] - 2:box[1] + 1] = True
        for k in range(12):
            got, want = Dv[k].cpu().numpy(), (np.where(grown, W[k], H[k]) if 6 <= k < 9 else W[k])
            assert np.array_equal(got, want), (k, _diff(got, want))
    finally:
        D._cabi.check(L.dlesm_halo_plan_destroy(plan))
