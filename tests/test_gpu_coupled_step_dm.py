"""GPU tests (-m gpu) of the coupled step on a decomposed grid, dlesm_nemolite_coupled_step_dm, and of the int halo exchange,
dlesm_halo_exchange_i32, in loop-back on one GPU: rank 0 is its own eight neighbours through depth-1
or depth-2 tables.  Each case compares the one call with its definition run through the separate public entries on the same
plan -- continuity, the ssha exchange, next_sshu / next_sshv, momentum, bc_open, the single-domain tracer entry of the scheme,
the exchange of the 5 + K outputs -- over whole sentinel-filled arrays: every cell of every output, inputs untouched.  Shapes:
260 x 10 (three wave tiles a row in both sweeps), 64 x 9 (one partial tile), 131 x 9 (the odd pitch: the five entries and the
one-cell-per-thread tracer kernels).  K = 0, 1, 5 (5: two tracer launches; over mailboxes of three fields the exchange takes
four turns), over the RCCL group and over the mailboxes with the RCCL group switched off underneath (dm_skip_parts = 1), with
an open-boundary plan and with a wet plan that has an inactive tile.  Also: a plan without messages, the refusals, the int
exchange, the Python wrappers."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

import momentum_numpy as M
import open_bc_numpy as B
import oracle_lib as O
import tracer_cases as TC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

PRM = (20.0, 0.00015, 50.0, 9.80665)          # rdt, cbfr, visc, g
METRICS = ("dx_t", "dy_t", "dx_u", "dy_u", "dx_v", "dy_v", "area_t", "area_u", "area_v")
INS = ("un", "vn", "ht", "hu", "hv", "sshn_t", "sshn_u", "sshn_v")
OUTS = ("ssha", "ssha_u", "ssha_v", "ua", "va")
MOM = ("un", "vn", "ht", "sshn_t", "hu", "sshn_u", "hv", "sshn_v", "ssha_u", "ssha_v")
SCHEMES = {"upwind": (0, "dlesm_tracer_step_f64"), "muscl": (1, "dlesm_tracer_step_muscl_f64"),
           "hancock": (2, "dlesm_tracer_step_hancock_f64")}
SSH_BC = 0.0625
WHO = b"dlesm_nemolite_coupled_step_dm"


@pytest.fixture(scope="module")
def D():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU: torch.cuda.is_available() is False")
    import dl_esm_inf_amd as d
    torch.cuda.set_device(0)
    d.parallel_init(0, 1, use_rccl=True)
    return d


def _p(t):
    return C.c_void_p(t.data_ptr())


def _ptrs(ts):
    return (C.c_void_p * max(len(ts), 1))(*[t.data_ptr() for t in ts])


def _R(D, box):
    return C.byref(D._cabi.Region(0, 0, *box))


def _vel(rng, shape):
    v = rng.normal(0.0, 0.3, shape)
    pick = rng.random(shape)
    v[pick < 0.15] = 0.0
    v[(pick >= 0.15) & (pick < 0.3)] = -0.0
    return v


def host_mask(rng, ld, ny, depth, kind):
    """"random": -1/0/1 with an open first internal column and an island across the east edge of the box, repaired for the
    open-boundary plan.  "wet" (260 x 10, depth 2): land and wet cells and a land patch over rows 4 and 5 (0-based) of the
    second wave tile of the box (columns 126..251) and column 252 -- the tile of row 4 then stores nothing but land ssha, and
    none of its cells lies in a strip the plan sends (rows 2, 3, 6, 7 and columns 2, 3, ld - 4, ld - 3)"""
    if kind == "wet":
        assert (ld, ny, depth) == (260, 10, 2)
        tm = rng.choice(np.array([0, 1, 1, 1], dtype=np.int32), size=(ny, ld))
        tm[4:6, 126:253] = 0
        return np.ascontiguousarray(tm)
    tm = rng.choice(np.array([-1, 0, 1, 1, 1, 1], dtype=np.int32), size=(ny, ld))
    tm[:, depth] = -1
    tm[ny // 3:ny // 3 + max(2, ny // 5), ld - 6:] = 0
    return B.repair(tm)


class Case:
    """raw (ny, ld) device arrays on a box with a ring of `depth` cells and a depth-`depth` loop-back plan.  Every double
    input and grid array carries the periodic halos of the plan (the halos a neighbour would hold), computed on the host by the
    oracle's exchange; the outputs are sentinels (ssha: distinct values, the caller's ring)."""

    def __init__(self, D, ld, ny, depth, k, seed, peer=0, tables=True, mask="random"):
        import torch
        from dm_overhead import loopback_tables
        self.D, self.L = D, D._cabi.lib()
        self.ld, self.ny, self.depth, self.k, self.peer = ld, ny, depth, k, peer
        self.box = (depth + 1, ld - depth, depth + 1, ny - depth)
        it = D._cabi.Region(ld - 2 * depth, ny - 2 * depth, *self.box)
        rng = np.random.default_rng(seed)
        self.tm = host_mask(rng, ld, ny, depth, mask)
        H = {n: _vel(rng, (ny, ld)) for n in ("un", "vn")}
        for n in ("ht", "hu", "hv"):
            H[n] = 10.0 + rng.random((ny, ld))
        for n in ("sshn_t", "sshn_u", "sshn_v"):
            H[n] = 0.1 * rng.normal(size=(ny, ld))
        G = {}
        for name in METRICS:
            a = 900.0 + 200.0 * rng.random((ny, ld))
            G[name] = a * 1000.0 if name.startswith("area") else a
        G["fcor_u"] = M.coriolis(40.0 + 20.0 * rng.random((ny, ld)), 7.292116e-5, np.pi / 180.0)
        G["fcor_v"] = M.coriolis(40.0 + 20.0 * rng.random((ny, ld)), 7.292116e-5, np.pi / 180.0)
        self.c_in, self.c_out = TC.tracers(rng, (ny, ld), k)
        self.t = loopback_tables(D, it, depth) if tables else D._cabi.CommTables()
        if tables:
            oc = O.Comms()
            C.memmove(C.byref(oc), C.byref(self.t), C.sizeof(oc))
            for a in list(H.values()) + list(G.values()) + self.c_in:
                assert O.exchange_all([a], [ld], [oc]) == 0
        self.Hi = H
        self.Ho = {"ssha": 1000.0 + rng.random((ny, ld))}
        for n in OUTS[1:]:
            self.Ho[n] = np.full((ny, ld), -7.0)

        def dev(a):
            return torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.dev = dev
        self.I = {n: dev(v) for n, v in H.items()}
        self.gdev = {n: dev(v) for n, v in G.items()}
        self.gdev["tmask"] = torch.from_numpy(self.tm).cuda()
        self.mg = D._cabi.MomentumGrid(**{n: self.gdev[n].data_ptr() for n in M.GRID_ARRAYS})
        self.ci = [dev(a) for a in self.c_in]
        self.plan = C.c_void_p()
        D._cabi.check(self.L.dlesm_halo_plan_create(C.byref(self.t), ld, ny, C.byref(self.plan)))
        if peer:
            from dl_esm_inf_amd import grid_mod
            grid_mod.connect_peers(types.SimpleNamespace(_halo_plan=self.plan), peer)
            self.L.dlesm_set_tuning(b"dm_skip_parts", 1)      # no RCCL group: only the mailboxes can move the halos
        self.obc = self.wet = None

    def outputs(self):
        return {n: self.dev(v) for n, v in self.Ho.items()}, [self.dev(a) for a in self.c_out]

    def make_obc(self):
        h = C.c_void_p()
        self.D._cabi.check(self.L.dlesm_obc_create(self.tm.ctypes.data, self.ld, self.ny, *[_R(self.D, self.box)] * 3,
                                                   C.byref(h)))
        self.obc = h
        return h

    def make_wet(self):
        h = C.c_void_p()
        self.D._cabi.check(self.L.dlesm_wet_plan_create(self.tm.ctypes.data, self.ld, self.ny, _R(self.D, self.box), C.byref(h)))
        self.wet = h
        return h

    def inputs_untouched(self):
        for n in INS:
            assert M.same(self.I[n].cpu().numpy(), self.Hi[n]), n
        for n in range(self.k):
            assert M.same(self.ci[n].cpu().numpy(), self.c_in[n]), n
        assert np.array_equal(self.gdev["tmask"].cpu().numpy(), self.tm)

    def close(self):
        self.L.dlesm_set_tuning(b"dm_skip_parts", 0)
        if self.obc is not None:
            self.L.dlesm_obc_destroy(self.obc)
        if self.wet is not None:
            self.L.dlesm_wet_plan_destroy(self.wet)
        self.D._cabi.check(self.L.dlesm_halo_plan_destroy(self.plan))


def tracer_entry(S, scheme, O_, co, prm):
    """step 4 of the definition: the single-domain entry of the scheme over tbox with params->rdt and the ssha just made"""
    if not S.k:
        return
    flow = {**S.I, "ssha": O_["ssha"]}
    fn = getattr(S.L, SCHEMES[scheme][1])
    S.D._cabi.check(fn(prm.rdt, S.ld, S.ny, *S.box, _p(S.gdev["tmask"]), _p(S.gdev["area_t"]), *[_p(flow[n]) for n in TC.FLOW],
                       _ptrs(S.ci), _ptrs(co), S.k, None))


def definition(S, scheme, O_, co, obc, ssh_bc, prm):
    """DESIGN.md section 6.13's definition on the plan, through the separate public entries; the last exchange in turns of the
    mailbox's field count over the mailboxes, as one aggregated exchange otherwise"""
    D, L, ck = S.D, S.L, S.D._cabi.check
    I, ld, ny, g, b = S.I, S.ld, S.ny, S.gdev, S.box
    ck(L.dlesm_continuity_f64(prm.rdt, ld, ny, *b, *[_p(I[n]) for n in ("sshn_t", "sshn_u", "sshn_v", "hu", "hv", "un", "vn")],
                              _p(g["area_t"]), _p(O_["ssha"]), None))
    ck(L.dlesm_halo_exchange_f64(S.plan, _p(O_["ssha"]), D._cabi.DIRS_ALL, None))
    ck(L.dlesm_next_sshu_f64(ld, ny, *b, _p(g["tmask"]), _p(g["area_t"]), _p(g["area_u"]), _p(O_["ssha"]), _p(O_["ssha_u"]),
                             None))
    ck(L.dlesm_next_sshv_f64(ld, ny, *b, _p(g["tmask"]), _p(g["area_t"]), _p(g["area_v"]), _p(O_["ssha"]), _p(O_["ssha_v"]),
                             None))
    ck(L.dlesm_momentum_f64(C.byref(prm), C.byref(S.mg), ld, ny, _R(D, b), _R(D, b),
                            *[_p((I if n in I else O_)[n]) for n in MOM], _p(O_["ua"]), _p(O_["va"]), None))
    if obc is not None:
        ck(L.dlesm_bc_open_f64(obc, C.byref(prm), ssh_bc, *[_p(I[n]) for n in ("hu", "sshn_u", "hv", "sshn_v", "sshn_t")],
                               _p(O_["ssha"]), _p(O_["ua"]), _p(O_["va"]), None))
    tracer_entry(S, scheme, O_, co, prm)
    fields = [O_[n] for n in OUTS] + list(co)
    turn = S.peer or len(fields)
    for n in range(0, len(fields), turn):
        ck(L.dlesm_halo_exchange_multi_f64(S.plan, _ptrs(fields[n:n + turn]), len(fields[n:n + turn]), D._cabi.DIRS_ALL, None))


def one_call(S, scheme, O_, co, obc, ssh_bc, prm, wet=None, boxes=None, plan=None, k=None, ci=None):
    tb, ub, vb = boxes or (S.box,) * 3
    k = S.k if k is None else k
    ci = S.ci if ci is None else ci
    return S.L.dlesm_nemolite_coupled_step_dm(
        S.plan if plan is None else plan, wet, scheme if isinstance(scheme, int) else SCHEMES[scheme][0], C.byref(prm),
        C.byref(S.mg), _p(S.gdev["area_t"]), S.ld, S.ny, _R(S.D, tb), _R(S.D, ub), _R(S.D, vb), obc, ssh_bc,
        *[_p(S.I[n]) for n in INS], *[_p(O_[n]) for n in OUTS], _ptrs(ci) if ci else None, _ptrs(co) if co else None, k, None)


def _compare(S, O1, c1, Od, cd, ssha_where=None):
    for n in OUTS:
        x, y = O1[n].cpu().numpy(), Od[n].cpu().numpy()
        if n == "ssha" and ssha_where is not None:
            x, y = x[ssha_where], y[ssha_where]
        assert M.same(x, y), (n, np.argwhere((x != y) & ~(np.isnan(x) & np.isnan(y)))[:5])
    for n in range(S.k):
        x, y = c1[n].cpu().numpy(), cd[n].cpu().numpy()
        assert M.same(x, y), ("tracer", n, np.argwhere(x != y)[:5])


def _halos_moved(S, a):
    """loop-back: the east halo columns hold the west internal columns, the north halo rows the south internal ones"""
    d, ld, ny = S.depth, S.ld, S.ny
    assert M.same(a[d:-d, ld - d:], a[d:-d, d:2 * d]) and M.same(a[ny - d:, d:-d], a[d:2 * d, d:-d])


def _check(D, ld, ny, depth, scheme, k, peer, with_obc=False, mask="random", wet=False):
    import torch
    S = Case(D, ld, ny, depth, k, ld * 31 + ny * 7 + depth + k, peer=peer, mask=mask)
    try:
        prm = D.psy.momentum_params(*PRM)
        obc = S.make_obc() if with_obc else None
        w = S.make_wet() if wet else None
        where = None
        if wet:
            tiles, active = C.c_longlong(), C.c_longlong()
            D._cabi.check(S.L.dlesm_wet_plan_counts(w, C.byref(tiles), C.byref(active)))
            assert 0 < active.value < tiles.value, (tiles.value, active.value)
            # section 6.9's contract: ssha is the definition's in every cell with T != 0 and in every cell outside tbox
            where = S.tm != 0
            xs, xe, ys, ye = S.box
            outside = np.ones((ny, ld), dtype=bool)
            outside[ys - 1:ye, xs - 1:xe] = False
            where |= outside
        (Od, cd), (O1, c1) = S.outputs(), S.outputs()
        definition(S, scheme, Od, cd, obc, SSH_BC, prm)
        rc = one_call(S, scheme, O1, c1, obc, SSH_BC, prm, wet=w)
        assert rc == 0, S.L.dlesm_last_error()
        torch.cuda.synchronize()
        assert S.L.dlesm_wait_timed_out(0) == 0
        _compare(S, O1, c1, Od, cd, ssha_where=where)
        S.inputs_untouched()
        got = O1["ua"].cpu().numpy()
        assert (got != -7.0).any()
        for a in [O1[n] for n in OUTS[(1 if wet else 0):]] + c1:
            _halos_moved(S, a.cpu().numpy())
        for n in range(k):
            inner = c1[n].cpu().numpy()[depth:-depth, depth:-depth]
            assert (inner != TC.SENTINEL).any() and (S.tm <= 0).any()
        if with_obc:
            nt, nu, nv = C.c_int(), C.c_int(), C.c_int()
            D._cabi.check(S.L.dlesm_obc_counts(obc, C.byref(nt), C.byref(nu), C.byref(nv)))
            assert nt.value > 0 and nu.value > 0
    finally:
        S.close()


CASES = [
    (260, 10, 2, "upwind", 1), (260, 10, 2, "muscl", 1), (260, 10, 2, "hancock", 5), (260, 10, 2, "hancock", 0),
    (260, 10, 1, "upwind", 5), (260, 10, 1, "muscl", 0),
    (64, 9, 2, "upwind", 5), (64, 9, 2, "muscl", 1), (64, 9, 2, "hancock", 1), (64, 9, 1, "upwind", 1),
    (131, 9, 2, "upwind", 1), (131, 9, 2, "muscl", 5), (131, 9, 2, "hancock", 1), (131, 9, 1, "upwind", 0),
    (131, 9, 1, "upwind", 5),
]


@pytest.mark.parametrize("peer", [0, 3])
@pytest.mark.parametrize("ld,ny,depth,scheme,k", CASES)
def test_one_call_equals_the_definition(D, ld, ny, depth, scheme, k, peer):
    """whole sentinel-filled arrays: every cell of the 5 + K outputs equals the definition's, inputs untouched, no wait gave
    up; peer = 3: the mailboxes connected for three fields (K = 5: four turns), the RCCL group switched off"""
    _check(D, ld, ny, depth, scheme, k, peer)


@pytest.mark.parametrize("ld,ny,depth,scheme,k,peer", [(260, 10, 2, "hancock", 1, 0), (260, 10, 2, "muscl", 2, 3),
                                                       (131, 9, 2, "muscl", 1, 0), (64, 9, 1, "upwind", 1, 3)])
def test_with_an_open_boundary_plan(D, ld, ny, depth, scheme, k, peer):
    _check(D, ld, ny, depth, scheme, k, peer, with_obc=True)


@pytest.mark.parametrize("peer", [0, 3])
def test_with_a_wet_plan_that_has_an_inactive_tile(D, peer):
    """ssha is compared where T != 0 and outside tbox (DESIGN.md section 6.9's contract), everything else in every cell"""
    _check(D, 260, 10, 2, "hancock", 2, peer, mask="wet", wet=True)


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("boxes", [None, ((37, 250, 5, 8), (40, 257, 3, 8), (3, 258, 4, 7))])
def test_plan_without_messages(D, k, boxes):
    """a plan of empty tables: dlesm_nemolite_step_wet_f64 followed by the tracer entry over tbox, for any boxes"""
    import torch
    S = Case(D, 260, 10, 2, k, 4242 + k, tables=False)
    try:
        prm = D.psy.momentum_params(*PRM)
        tb, ub, vb = boxes or (S.box,) * 3
        (Os, cs), (O1, c1) = S.outputs(), S.outputs()
        D._cabi.check(S.L.dlesm_nemolite_step_wet_f64(None, C.byref(prm), C.byref(S.mg), _p(S.gdev["area_t"]), S.ld, S.ny,
                                                      _R(D, tb), _R(D, ub), _R(D, vb), None, 0.0, *[_p(S.I[n]) for n in INS],
                                                      *[_p(Os[n]) for n in OUTS], None))
        flow = {**S.I, "ssha": Os["ssha"]}
        D._cabi.check(S.L.dlesm_tracer_step_hancock_f64(prm.rdt, S.ld, S.ny, *tb, _p(S.gdev["tmask"]), _p(S.gdev["area_t"]),
                                                        *[_p(flow[n]) for n in TC.FLOW], _ptrs(S.ci), _ptrs(cs), k, None))
        assert one_call(S, "hancock", O1, c1, None, 0.0, prm, boxes=(tb, ub, vb)) == 0, S.L.dlesm_last_error()
        torch.cuda.synchronize()
        _compare(S, O1, c1, Os, cs)
        assert all((c.cpu().numpy() != TC.SENTINEL).any() for c in c1)
    finally:
        S.close()


def test_refusals(D):
    """DLESM_EINVAL naming the entry, before anything is launched or exchanged -- every output stays at its sentinel"""
    import torch
    from dm_overhead import loopback_tables
    S2, S1 = Case(D, 64, 12, 2, 1, 5), Case(D, 64, 12, 1, 1, 6)
    L = S2.L
    other = C.c_void_p()
    D._cabi.check(L.dlesm_halo_plan_create(C.byref(loopback_tables(D, D._cabi.Region(62, 8, 3, 64, 3, 10), 2)), 66, 12,
                                           C.byref(other)))
    try:
        prm = D.psy.momentum_params(*PRM)
        (O2, c2), (O1, c1) = S2.outputs(), S1.outputs()
        nine = [c2[0]] * 9
        cases = [
            ("a limited scheme on a depth-1 plan", S1, O1, c1, dict(scheme="muscl"), b"depth-1"),
            ("scheme = 3", S2, O2, c2, dict(scheme=3), b"scheme 3"),
            ("ntracers = 9", S2, O2, nine, dict(scheme="upwind", k=9, ci=[S2.ci[0]] * 9), b"9 tracers"),
            ("c_out is ua", S2, O2, [O2["ua"]], dict(scheme="hancock"), b"overlap"),
            ("a null plan", S2, O2, c2, dict(scheme="hancock", plan=C.c_void_p(0)), b"null plan"),
            ("a plan of other extents", S2, O2, c2, dict(scheme="hancock", plan=other), b"66x12"),
            ("unequal boxes", S2, O2, c2, dict(scheme="hancock", boxes=(S2.box, S2.box, (3, 61, 3, 10))), b"one box"),
        ]
        got = []
        for what, S, O_, co, kw, msg in cases:
            scheme = kw.pop("scheme")
            rc = one_call(S, scheme, O_, co, None, 0.0, prm, **kw)
            err = L.dlesm_last_error()
            got.append((what, rc, WHO in err and msg in err, err))
        assert all(rc == D._cabi.EINVAL and ok for _, rc, ok, _ in got), got
        torch.cuda.synchronize()
        for S, O_, co in ((S2, O2, c2), (S1, O1, c1)):
            for n in OUTS:
                assert M.same(O_[n].cpu().numpy(), S.Ho[n]), n
            assert (co[0].cpu().numpy() == TC.SENTINEL).all()
            S.inputs_untouched()
    finally:
        L.dlesm_halo_plan_destroy(other)
        S2.close()
        S1.close()


# ---- dlesm_halo_exchange_i32 -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("peer", [0, 1])
@pytest.mark.parametrize("ld,ny,depth", [(64, 9, 1), (260, 10, 2), (131, 9, 2)])
def test_halo_exchange_i32(D, ld, ny, depth, peer):
    """j*ld + i with some cells negative and the two extreme int32 values in sent cells: the array equals, cast to int, what
    dlesm_halo_exchange_f64 leaves on the double copy; the received halos hold the opposite internal strips; cells no message
    covers are unchanged (a halo ring wider than the plan's depth is part of them)"""
    import torch
    from dm_overhead import loopback_tables
    L = D._cabi.lib()
    pad = 1                                                  # one more ring cell than the plan exchanges
    d = depth
    box = (d + pad + 1, ld - d - pad, d + pad + 1, ny - d - pad)
    t = loopback_tables(D, D._cabi.Region(ld - 2 * (d + pad), ny - 2 * (d + pad), *box), d)
    plan = C.c_void_p()
    D._cabi.check(L.dlesm_halo_plan_create(C.byref(t), ld, ny, C.byref(plan)))
    if peer:
        from dl_esm_inf_amd import grid_mod
        grid_mod.connect_peers(types.SimpleNamespace(_halo_plan=plan), peer)
        L.dlesm_set_tuning(b"dm_skip_parts", 1)
    try:
        jj, ii = np.mgrid[0:ny, 0:ld]
        a = (jj * ld + ii).astype(np.int32)
        a[(ii + jj) % 3 == 0] *= -1
        lo = d + pad                                          # 0-based first internal row / column: a sent cell
        a[lo, lo] = np.iinfo(np.int32).min
        a[ny - lo - 1, ld - lo - 1] = np.iinfo(np.int32).max
        f32, f64 = torch.from_numpy(a).cuda(), torch.from_numpy(a.astype(np.float64)).cuda()
        D._cabi.check(L.dlesm_halo_exchange_f64(plan, _p(f64), D._cabi.DIRS_ALL, None))
        assert L.dlesm_halo_exchange_i32(plan, _p(f32), None) == 0, L.dlesm_last_error()
        torch.cuda.synchronize()
        assert L.dlesm_wait_timed_out(0) == 0
        got, want = f32.cpu().numpy(), f64.cpu().numpy()
        assert got.dtype == np.int32 and np.array_equal(got.astype(np.float64), want)
        # the received halos: the opposite internal strips, corners included
        xs, xe, ys, ye = [v - 1 for v in box]                # 0-based inclusive
        cols = np.r_[xe - d + 1:xe + 1, xs:xe + 1, xs:xs + d]
        rows = np.r_[ye - d + 1:ye + 1, ys:ye + 1, ys:ys + d]
        assert np.array_equal(got[ys - d:ye + d + 1, xs - d:xe + d + 1], a[np.ix_(rows, cols)])
        covered = np.zeros((ny, ld), dtype=bool)
        covered[ys - d:ye + d + 1, xs - d:xe + d + 1] = True
        covered[ys:ye + 1, xs:xe + 1] = False
        assert np.array_equal(got[~covered], a[~covered]) and (got[covered] != a[covered]).any()
        assert got[ye + 1, xe + 1] == np.iinfo(np.int32).min and got[ys - 1, xs - 1] == np.iinfo(np.int32).max
    finally:
        L.dlesm_set_tuning(b"dm_skip_parts", 0)
        D._cabi.check(L.dlesm_halo_plan_destroy(plan))


def test_halo_exchange_i32_without_messages_and_refusals(D):
    import torch
    L = D._cabi.lib()
    t = D._cabi.CommTables()
    plan = C.c_void_p()
    D._cabi.check(L.dlesm_halo_plan_create(C.byref(t), 64, 9, C.byref(plan)))
    try:
        a = np.arange(64 * 9, dtype=np.int32).reshape(9, 64) - 100
        f = torch.from_numpy(a).cuda()
        assert L.dlesm_halo_exchange_i32(plan, _p(f), None) == 0, L.dlesm_last_error()
        torch.cuda.synchronize()
        assert np.array_equal(f.cpu().numpy(), a)
        assert L.dlesm_halo_exchange_i32(None, _p(f), None) == D._cabi.EINVAL
        assert b"dlesm_halo_exchange_i32" in L.dlesm_last_error()
        assert L.dlesm_halo_exchange_i32(plan, None, None) == D._cabi.EINVAL
    finally:
        D._cabi.check(L.dlesm_halo_plan_destroy(plan))


def test_halo_exchange_i32_refuses_a_stream_that_is_being_captured(D):
    """the first use allocates the plan's scratch: DLESM_EINVAL before anything is put into the capture, the field untouched"""
    import torch
    from dm_overhead import loopback_tables
    L = D._cabi.lib()
    t = loopback_tables(D, D._cabi.Region(62, 7, 2, 63, 2, 8), 1)
    plan = C.c_void_p()
    D._cabi.check(L.dlesm_halo_plan_create(C.byref(t), 64, 9, C.byref(plan)))
    try:
        a = np.arange(64 * 9, dtype=np.int32).reshape(9, 64) - 100
        f = torch.from_numpy(a).cuda()
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
            rc = L.dlesm_halo_exchange_i32(plan, _p(f), C.c_void_p(s.cuda_stream))
            err = L.dlesm_last_error()
        assert rc == D._cabi.EINVAL and b"dlesm_halo_exchange_i32" in err and b"captured" in err, (rc, err)
        torch.cuda.synchronize()
        assert np.array_equal(f.cpu().numpy(), a)
        del graph
    finally:
        D._cabi.check(L.dlesm_halo_plan_destroy(plan))


# ---- through the Python wrappers ----------------------------------------------------------------------------------------
def _tracer_fields(D, g, arrays):
    import torch
    out = []
    for a in arrays:
        f = D.r2d_field(g, D.GO_T_POINTS)
        f.data.copy_(torch.from_numpy(a))
        out.append(f)
    return out


def test_python_wrapper_on_one_rank(D):
    """on a one-rank grid decomposed with halo_width = 2 invoke_nemolite_coupled_step_dm equals invoke_nemolite_step followed
    by invoke_tracer_step_hancock"""
    import torch
    import test_gpu_nemolite_step_dm as DM
    g, H, F, F2 = DM._pygrid(D, 200, 12, halo_width=2)
    rng = np.random.default_rng(3)
    c = [1.0 + n + rng.random((g.ny, g.nx)) for n in range(2)]
    sent = [np.full_like(a, TC.SENTINEL) for a in c]
    Ci, Co, Co2 = _tracer_fields(D, g, c), _tracer_fields(D, g, sent), _tracer_fields(D, g, sent)
    prm = D.psy.momentum_params(*PRM)
    D.psy.invoke_nemolite_step(prm, *[F[n] for n in OUTS], *[F[n] for n in INS])
    D.psy.invoke_tracer_step_hancock(prm.rdt, Co, Ci, F["ssha"], *[F[n] for n in INS])
    D.psy.invoke_nemolite_coupled_step_dm(prm, "hancock", Co2, Ci, *[F2[n] for n in OUTS], *[F2[n] for n in INS])
    torch.cuda.synchronize()
    for n in H:
        assert M.same(F2[n].get_data(), F[n].get_data()), n
    for n in range(2):
        assert M.same(Co2[n].get_data(), Co[n].get_data()), n
        assert (Co[n].get_data() != TC.SENTINEL).any()
    assert not M.same(F["ua"].get_data(), H["ua"])


def test_python_wrapper_refusals(D):
    """halo_width = 1 with "muscl": GoceanStop naming halo_width = 2; halo_width = 3: GoceanStop; no Coriolis parameter:
    GoceanStop; nothing is written"""
    import torch
    import test_gpu_nemolite_step_dm as DM
    prm = D.psy.momentum_params(*PRM)
    made = []

    def call(hw, scheme, coriolis=True):
        g, H, F, _ = DM._pygrid(D, 64, 32, halo_width=hw, coriolis=coriolis)
        c = [np.ones((g.ny, g.nx))]
        Ci, Co = _tracer_fields(D, g, c), _tracer_fields(D, g, [np.full_like(c[0], TC.SENTINEL)])
        made.append((H, F, Co))
        D.psy.invoke_nemolite_coupled_step_dm(prm, scheme, Co, Ci, *[F[n] for n in OUTS], *[F[n] for n in INS])
    with pytest.raises(D._cabi.GoceanStop, match="halo_width = 2"):
        call(1, "muscl")
    with pytest.raises(D._cabi.GoceanStop, match="halo_width 3"):
        call(3, "upwind")
    with pytest.raises(D._cabi.GoceanStop, match="Coriolis"):
        call(2, "hancock", coriolis=False)
    torch.cuda.synchronize()
    assert len(made) == 3
    for H, F, Co in made:
        for n in OUTS:
            assert M.same(F[n].get_data(), H[n]), n
        assert (Co[0].get_data() == TC.SENTINEL).all()


def test_exchange_mask_halos_on_one_rank(D):
    """a plan without messages: grid.tmask stays as it was, and a cached wet_plan is dropped"""
    import test_gpu_nemolite_step_dm as DM
    from dl_esm_inf_amd import grid_mod
    g, _, _, _ = DM._pygrid(D, 64, 32, halo_width=1)
    before = g.tmask.copy()
    assert (before == 0).any() and (before > 0).any()
    D.psy.wet_plan(g)
    D.psy.open_boundary(g)
    assert g._wet is not None and g._obc is not None
    grid_mod.exchange_mask_halos(g)
    assert g._wet is None and g._obc is None
    assert g.tmask.dtype == np.int32 and np.array_equal(g.tmask, before)
    assert np.array_equal(g.tmask_device.cpu().numpy(), before)
    assert D.psy.wet_plan(g).handle
