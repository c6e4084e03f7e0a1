"""GPU tests (-m gpu) of the one-call NEMOLite2D-class time step on a decomposed grid, dlesm_nemolite_step_dm (DESIGN.md
section 6.8), in loop-back on one GPU: rank 0 is its own eight neighbours through depth-1 tables.  Each case compares the one
call with its definition on the same plan -- continuity, the ssha exchange, next_sshu / next_sshv, momentum, bc_open, the
exchange of the five outputs -- over whole sentinel-filled arrays: every cell of all five outputs, inputs untouched.  Paths:
the sweep (even pitch), the five entries (odd pitch, unaligned bases, the HOOK key nemo_step_kernel); with and without an
open-boundary plan; over the RCCL group and over the mailboxes with the RCCL group switched off underneath (dm_skip_parts = 1);
a 20-step time loop; one step at 8192^2.  Also: a plan without messages is dlesm_nemolite_step_f64; the refusals; the Python
wrapper."""
import ctypes as C
import math
import os
import sys
import types

import numpy as np
import pytest

import momentum_numpy as M
import open_bc_numpy as B
import oracle_lib as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

PRM = (20.0, 0.00015, 50.0, 9.80665)          # rdt, cbfr, visc, g
METRICS = ("dx_t", "dy_t", "dx_u", "dy_u", "dx_v", "dy_v", "area_t", "area_u", "area_v")
INS = ("un", "vn", "ht", "hu", "hv", "sshn_t", "sshn_u", "sshn_v")
OUTS = ("ssha", "ssha_u", "ssha_v", "ua", "va")
MOM = ("un", "vn", "ht", "sshn_t", "hu", "sshn_u", "hv", "sshn_v", "ssha_u", "ssha_v")
SSH_BC = 0.0625


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


def _R(D, box):
    return C.byref(D._cabi.Region(0, 0, *box))


def _vel(rng, shape):
    v = rng.normal(0.0, 0.3, shape)
    pick = rng.random(shape)
    v[pick < 0.15] = 0.0
    v[(pick >= 0.15) & (pick < 0.3)] = -0.0
    return v


def _mask(rng, ld, ny):
    """random -1/0/1, an open west column, an island across the east edge of the box; repaired for the open-boundary plan"""
    tm = rng.choice(np.array([-1, 0, 1, 1, 1, 1], dtype=np.int32), size=(ny, ld))
    tm[:, 1] = -1
    tm[ny // 3:ny // 3 + max(2, ny // 5), ld - 6:] = 0
    return B.repair(tm)


class Case:
    """raw (ny, ld) device arrays on a box with a one-cell ring and a depth-1 loop-back plan.  Every double input and
    grid array carries the periodic halos of the plan (the halos a neighbour would hold), computed on the host by the oracle's
    exchange; the outputs are sentinels (ssha: distinct values, the caller's ring)."""

    def __init__(self, D, ld, ny, seed, shift=0, peer=0, mask=True, tables=True):
        import torch
        from dm_overhead import loopback_tables
        self.D, self.L = D, D._cabi.lib()
        self.ld, self.ny = ld, ny
        self.box = (2, ld - 1, 2, ny - 1)
        it = D._cabi.Region(ld - 2, ny - 2, *self.box)
        rng = np.random.default_rng(seed)
        self.tm = _mask(rng, ld, ny) if mask else np.ones((ny, ld), dtype=np.int32)
        H = {k: _vel(rng, (ny, ld)) for k in ("un", "vn")}
        for k in ("ht", "hu", "hv"):
            H[k] = 10.0 + rng.random((ny, ld))
        for k in ("sshn_t", "sshn_u", "sshn_v"):
            H[k] = 0.1 * rng.normal(size=(ny, ld))
        G = {}
        for name in METRICS:
            a = 900.0 + 200.0 * rng.random((ny, ld))
            G[name] = a * 1000.0 if name.startswith("area") else a
        G["fcor_u"] = M.coriolis(40.0 + 20.0 * rng.random((ny, ld)), 7.292116e-5, math.pi / 180.0)
        G["fcor_v"] = M.coriolis(40.0 + 20.0 * rng.random((ny, ld)), 7.292116e-5, math.pi / 180.0)
        self.t = loopback_tables(D, it, 1) if tables else D._cabi.CommTables()
        if tables:
            oc = O.Comms()
            C.memmove(C.byref(oc), C.byref(self.t), C.sizeof(oc))
            for a in list(H.values()) + list(G.values()):
                assert O.exchange_all([a], [ld], [oc]) == 0
        self.Hi = H
        self.Ho = {"ssha": 1000.0 + rng.random((ny, ld))}
        for k in OUTS[1:]:
            self.Ho[k] = np.full((ny, ld), -7.0)

        def dev(a):
            t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            if shift:
                t = torch.cat([torch.zeros(1, dtype=t.dtype, device="cuda"), t.flatten()])[1:].view(a.shape)
            return t
        self.I = {k: dev(v) for k, v in H.items()}
        self.gdev = {k: dev(v) for k, v in G.items()}
        self.gdev["tmask"] = torch.from_numpy(self.tm).cuda()
        self.mg = D._cabi.MomentumGrid(**{k: self.gdev[k].data_ptr() for k in M.GRID_ARRAYS})
        self.dev = dev
        self.plan = C.c_void_p()
        D._cabi.check(self.L.dlesm_halo_plan_create(C.byref(self.t), ld, ny, C.byref(self.plan)))
        self.peer = peer
        if peer:
            from dl_esm_inf_amd import grid_mod
            grid_mod.connect_peers(types.SimpleNamespace(_halo_plan=self.plan), peer)
            self.L.dlesm_set_tuning(b"dm_skip_parts", 1)      # no RCCL group: only the mailboxes can move the halos
        self.obc = None

    def outputs(self):
        return {k: self.dev(v) for k, v in self.Ho.items()}

    def make_obc(self):
        h = C.c_void_p()
        self.D._cabi.check(self.L.dlesm_obc_create(self.tm.ctypes.data, self.ld, self.ny, *[_R(self.D, self.box)] * 3,
                                                   C.byref(h)))
        self.obc = h
        return h

    def close(self):
        self.L.dlesm_set_tuning(b"dm_skip_parts", 0)
        self.L.dlesm_set_tuning(b"nemo_step_kernel", 0)
        if self.obc is not None:
            self.L.dlesm_obc_destroy(self.obc)
        self.D._cabi.check(self.L.dlesm_halo_plan_destroy(self.plan))


def definition(S, I, O_, obc, ssh_bc, prm, boxes=None):
    """DESIGN.md section 6.8's definition on the plan: continuity, the ssha exchange, next_ssh*, momentum, bc_open, the exchange
    of the five outputs (in turns of the mailbox's field count over the mailboxes, as one aggregated exchange otherwise)"""
    D, L, ck = S.D, S.L, S.D._cabi.check
    tb, ub, vb = boxes or (S.box,) * 3
    ld, ny, g = S.ld, S.ny, S.gdev
    ck(L.dlesm_continuity_f64(prm.rdt, ld, ny, *tb, *[_p(I[k]) for k in ("sshn_t", "sshn_u", "sshn_v", "hu", "hv", "un", "vn")],
                              _p(g["area_t"]), _p(O_["ssha"]), None))
    ck(L.dlesm_halo_exchange_f64(S.plan, _p(O_["ssha"]), D._cabi.DIRS_ALL, None))
    ck(L.dlesm_next_sshu_f64(ld, ny, *ub, _p(g["tmask"]), _p(g["area_t"]), _p(g["area_u"]), _p(O_["ssha"]), _p(O_["ssha_u"]),
                             None))
    ck(L.dlesm_next_sshv_f64(ld, ny, *vb, _p(g["tmask"]), _p(g["area_t"]), _p(g["area_v"]), _p(O_["ssha"]), _p(O_["ssha_v"]),
                             None))
    ck(L.dlesm_momentum_f64(C.byref(prm), C.byref(S.mg), ld, ny, _R(D, ub), _R(D, vb),
                            *[_p((I if k in I else O_)[k]) for k in MOM], _p(O_["ua"]), _p(O_["va"]), None))
    if obc is not None:
        ck(L.dlesm_bc_open_f64(obc, C.byref(prm), ssh_bc, *[_p(I[k]) for k in ("hu", "sshn_u", "hv", "sshn_v", "sshn_t")],
                               _p(O_["ssha"]), _p(O_["ua"]), _p(O_["va"]), None))
    turn = S.peer or 5
    for k in range(0, 5, turn):
        names = OUTS[k:k + turn]
        arr = (C.c_void_p * len(names))(*[O_[n].data_ptr() for n in names])
        ck(L.dlesm_halo_exchange_multi_f64(S.plan, arr, len(names), D._cabi.DIRS_ALL, None))


def one_call(S, I, O_, obc, ssh_bc, prm, boxes=None, plan=None):
    tb, ub, vb = boxes or (S.box,) * 3
    return S.L.dlesm_nemolite_step_dm(S.plan if plan is None else plan, C.byref(prm), C.byref(S.mg), _p(S.gdev["area_t"]),
                                      S.ld, S.ny, _R(S.D, tb), _R(S.D, ub), _R(S.D, vb), obc, ssh_bc,
                                      *[_p(I[k]) for k in INS], *[_p(O_[k]) for k in OUTS], None)


def _same_outputs(a, b, what=""):
    for k in OUTS:
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        assert M.same(x, y), (what, k, np.argwhere((x != y) & ~(np.isnan(x) & np.isnan(y)))[:5])


@pytest.mark.parametrize("peer", [0, 3, 5])
@pytest.mark.parametrize("with_obc", [False, True])
@pytest.mark.parametrize("ld,ny,shift,kernel", [
    (300, 70, 0, 0),     # even pitch, aligned: the sweep
    (130, 21, 0, 0),     # even pitch, a short tile
    (301, 41, 0, 0),     # odd pitch: the five entries
    (256, 33, 1, 0),     # bases 8 bytes off a 16-byte boundary: the five entries
    (300, 70, 0, 1),     # the HOOK key nemo_step_kernel = 1: the five entries
    (6, 5, 0, 0),        # a 4 x 3 box
])
def test_one_call_equals_the_definition(D, ld, ny, shift, kernel, with_obc, peer):
    """whole sentinel-filled arrays: every cell of the five outputs equals the definition's, inputs untouched; peer: the
    mailboxes connected for that many fields (3: the exchange in two turns), the RCCL group switched off"""
    import torch
    S = Case(D, ld, ny, ld * 31 + ny + shift, shift=shift, peer=peer)
    try:
        prm = D.psy.momentum_params(*PRM)
        obc = S.make_obc() if with_obc else None
        S.L.dlesm_set_tuning(b"nemo_step_kernel", kernel)
        Od, O1 = S.outputs(), S.outputs()
        definition(S, S.I, Od, obc, SSH_BC, prm)
        rc = one_call(S, S.I, O1, obc, SSH_BC, prm)
        assert rc == 0, S.L.dlesm_last_error()
        torch.cuda.synchronize()
        _same_outputs(O1, Od)
        for k in INS:
            assert M.same(S.I[k].cpu().numpy(), S.Hi[k]), k
        got = O1["ssha"].cpu().numpy()
        assert not M.same(got, S.Ho["ssha"])
        # the halos moved: the east halo column holds the west internal column (loop-back), the north row the south one
        assert M.same(got[1:-1, ld - 1], got[1:-1, 1]) and M.same(got[ny - 1, 1:-1], got[1, 1:-1])
        if with_obc and ld > 8:
            nt, nu, nv = C.c_int(), C.c_int(), C.c_int()
            D._cabi.check(S.L.dlesm_obc_counts(obc, C.byref(nt), C.byref(nu), C.byref(nv)))
            assert nt.value > 0 and nu.value > 0
    finally:
        S.close()


@pytest.mark.parametrize("peer", [0, 3])
@pytest.mark.parametrize("ld,ny", [(258, 66), (131, 40)])
def test_time_loop(D, ld, ny, peer):
    """20 steps of the one call with the rotation (un, vn, sshn_*) <-> (ua, va, ssha*), a tidal ssh_bc on an open column,
    against the definition run on its own copies: every array after every step"""
    import torch
    S = Case(D, ld, ny, 77 + ld, peer=peer)
    try:
        prm = D.psy.momentum_params(*PRM)
        obc = S.make_obc()
        A = {**{k: S.I[k].clone() for k in INS}, **S.outputs()}
        Bd = {**{k: S.I[k].clone() for k in INS}, **S.outputs()}
        omega = 2.0 * math.pi / 43200.0
        for step in range(20):
            ssh_bc = D.psy.tide_ssh(0.1, omega, (step + 1) * PRM[0])
            definition(S, Bd, Bd, obc, ssh_bc, prm)
            assert one_call(S, A, A, obc, ssh_bc, prm) == 0, S.L.dlesm_last_error()
            torch.cuda.synchronize()
            for k in A:
                x, y = A[k].cpu().numpy(), Bd[k].cpu().numpy()
                assert M.same(x, y), (step, k)
            for X in (A, Bd):
                for a, b in (("un", "ua"), ("vn", "va"), ("sshn_t", "ssha"), ("sshn_u", "ssha_u"), ("sshn_v", "ssha_v")):
                    X[a], X[b] = X[b], X[a]
        assert np.isfinite(A["sshn_t"].cpu().numpy()).all()
    finally:
        S.close()


def test_8192_whole_fields(D):
    """one step on an 8192^2 tile (the sweep) with an open-boundary plan, against the definition, whole arrays on the device"""
    import torch
    n = 8192
    ld = ny = n + 2
    S = Case.__new__(Case)
    S.D, S.L, S.ld, S.ny, S.box, S.peer, S.obc = D, D._cabi.lib(), ld, ny, (2, n + 1, 2, n + 1), 0, None
    from dm_overhead import loopback_tables
    S.t = loopback_tables(D, D._cabi.Region(n, n, *S.box), 1)
    S.plan = C.c_void_p()
    D._cabi.check(S.L.dlesm_halo_plan_create(C.byref(S.t), ld, ny, C.byref(S.plan)))
    try:
        gen = torch.Generator(device="cuda")
        gen.manual_seed(8192)

        def rnd(lo, span):
            return lo + span * torch.rand((ny, ld), dtype=torch.float64, device="cuda", generator=gen)
        S.tm = np.ones((ny, ld), dtype=np.int32)
        S.tm[:, 0] = S.tm[:, -1] = 0
        S.tm[:, 1] = -1                                            # an open west column
        S.tm[3000:3100, n - 40:] = 0                               # an island across the east edge
        S.gdev = {k: rnd(900.0, 200.0) * (1000.0 if k.startswith("area") else 1.0) for k in METRICS}
        S.gdev["fcor_u"], S.gdev["fcor_v"] = rnd(-1e-4, 2e-4), rnd(-1e-4, 2e-4)
        S.gdev["tmask"] = torch.from_numpy(S.tm).cuda()
        S.mg = D._cabi.MomentumGrid(**{k: S.gdev[k].data_ptr() for k in M.GRID_ARRAYS})
        I = {"un": rnd(-0.3, 0.6), "vn": rnd(-0.3, 0.6)}
        for k in ("ht", "hu", "hv"):
            I[k] = rnd(10.0, 1.0)
        for k in ("sshn_t", "sshn_u", "sshn_v"):
            I[k] = rnd(-0.1, 0.2)
        doubles = list(I.values()) + [v for k, v in S.gdev.items() if k != "tmask"]
        for a in doubles:                                          # the halos a neighbour would hold: the plan's own exchange
            D._cabi.check(S.L.dlesm_halo_exchange_f64(S.plan, _p(a), D._cabi.DIRS_ALL, None))
        O1 = {"ssha": rnd(1000.0, 1.0)}
        for k in OUTS[1:]:
            O1[k] = torch.full((ny, ld), -7.0, dtype=torch.float64, device="cuda")
        Od = {k: v.clone() for k, v in O1.items()}
        prm = D.psy.momentum_params(*PRM)
        obc = S.make_obc()
        definition(S, I, Od, obc, SSH_BC, prm)
        assert one_call(S, I, O1, obc, SSH_BC, prm) == 0, S.L.dlesm_last_error()
        torch.cuda.synchronize()
        for k in OUTS:
            same = bool(torch.equal(O1[k].view(torch.int64), Od[k].view(torch.int64)))
            assert same, (k, int((O1[k] != Od[k]).sum()))
        assert bool((O1["ua"] != -7.0).any())
    finally:
        S.close()


@pytest.mark.parametrize("with_obc", [False, True])
@pytest.mark.parametrize("boxes", [None, ((37, 250, 5, 60), (40, 298, 2, 69), (2, 299, 9, 50))])
def test_plan_without_messages_is_the_single_domain_call(D, boxes, with_obc):
    """a plan of empty tables: the call is dlesm_nemolite_step_f64, bit for bit, for any boxes (unequal ones included)"""
    import torch
    S = Case(D, 300, 70, 4242, tables=False)
    try:
        prm = D.psy.momentum_params(*PRM)
        obc = S.make_obc() if with_obc else None
        tb, ub, vb = boxes or (S.box,) * 3
        Os, O1 = S.outputs(), S.outputs()
        D._cabi.check(S.L.dlesm_nemolite_step_f64(C.byref(prm), C.byref(S.mg), _p(S.gdev["area_t"]), S.ld, S.ny, _R(D, tb),
                                                  _R(D, ub), _R(D, vb), obc, SSH_BC, *[_p(S.I[k]) for k in INS],
                                                  *[_p(Os[k]) for k in OUTS], None))
        assert one_call(S, S.I, O1, obc, SSH_BC, prm, boxes=(tb, ub, vb)) == 0, S.L.dlesm_last_error()
        torch.cuda.synchronize()
        _same_outputs(O1, Os)
    finally:
        S.close()


def test_refusals(D):
    """a depth-2 plan, unequal boxes, aliasing, a null plan, an open-boundary plan of other extents: DLESM_EINVAL with its
    message before anything is launched or exchanged -- every array untouched"""
    import torch
    from dm_overhead import loopback_tables
    S = Case(D, 64, 24, 5)
    L = S.L
    t2 = loopback_tables(D, D._cabi.Region(60, 20, 3, 62, 3, 22), 2)
    plan2, other = C.c_void_p(), C.c_void_p()
    D._cabi.check(L.dlesm_halo_plan_create(C.byref(t2), 64, 24, C.byref(plan2)))
    try:
        prm = D.psy.momentum_params(*PRM)
        O_ = S.outputs()
        cases = [
            (dict(plan=plan2), b"depth-2"),
            (dict(boxes=(S.box, S.box, (2, 62, 2, 22))), b"one box"),
            (dict(plan=C.c_void_p(0)), b"null plan"),
        ]
        got = []
        for kw, msg in cases:
            rc = one_call(S, S.I, O_, None, 0.0, prm, **kw)
            got.append((rc, msg in L.dlesm_last_error(), L.dlesm_last_error()))
        alias = dict(O_)
        alias["ua"] = O_["ssha"]
        rc = one_call(S, S.I, alias, None, 0.0, prm)
        got.append((rc, b"overlap" in L.dlesm_last_error(), L.dlesm_last_error()))
        alias = dict(O_)
        alias["va"] = S.I["vn"]
        rc = one_call(S, S.I, alias, None, 0.0, prm)
        got.append((rc, b"overlaps the input vn" in L.dlesm_last_error(), L.dlesm_last_error()))
        tm2 = np.ones((24, 66), dtype=np.int32)
        D._cabi.check(L.dlesm_obc_create(tm2.ctypes.data, 66, 24, *[_R(D, (2, 64, 2, 23))] * 3, C.byref(other)))
        rc = one_call(S, S.I, O_, other, 0.0, prm)
        got.append((rc, b"open-boundary plan was made for 66x24" in L.dlesm_last_error(), L.dlesm_last_error()))
        mg = S.mg
        S.mg = D._cabi.MomentumGrid(**{k: (0 if k == "fcor_v" else S.gdev[k].data_ptr()) for k in M.GRID_ARRAYS})
        rc = one_call(S, S.I, O_, None, 0.0, prm)
        S.mg = mg
        got.append((rc, b"Coriolis" in L.dlesm_last_error(), L.dlesm_last_error()))
        assert all(rc == D._cabi.EINVAL and ok for rc, ok, _ in got), got
        torch.cuda.synchronize()
        for k in OUTS:
            assert M.same(O_[k].cpu().numpy(), S.Ho[k]), k
        for k in INS:
            assert M.same(S.I[k].cpu().numpy(), S.Hi[k]), k
    finally:
        if other:
            S.L.dlesm_obc_destroy(other)
        S.close()
        L.dlesm_halo_plan_destroy(plan2)


def _pygrid(D, nx, ny, halo_width=1, coriolis=True):
    import torch
    os.environ["DL_ESM_ALIGNMENT"] = "64"
    g = D.grid_type(D.GO_ARAKAWA_C, (1, 1, 2), D.GO_OFFSET_NE)
    g.decompose(nx, ny, halo_width=halo_width)
    rng = np.random.default_rng(nx + ny)
    user = B.repair(rng.choice(np.array([-1, 0, 1, 1, 1], dtype=np.int32), size=(ny + 2, nx + 2)))
    D.grid_init(g, 1000.0, 1000.0, tmask=user if halo_width == 1 else None)
    os.environ.pop("DL_ESM_ALIGNMENT", None)
    if coriolis:
        g.gphiu = 40.0 + 20.0 * rng.random((g.ny, g.nx))
        g.gphiv = 40.0 + 20.0 * rng.random((g.ny, g.nx))
        D.psy.coriolis(g)
    T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
    pts = {"ssha": T, "sshn_t": T, "ht": T, "sshn_u": U, "ssha_u": U, "un": U, "ua": U, "hu": U,
           "sshn_v": V, "ssha_v": V, "vn": V, "va": V, "hv": V}
    H = {k: (10.0 + rng.random((g.ny, g.nx)) if k in ("ht", "hu", "hv") else 0.1 * rng.normal(size=(g.ny, g.nx)))
         for k in pts}
    F, F2 = {}, {}
    for k, p in pts.items():
        F[k], F2[k] = D.r2d_field(g, p), D.r2d_field(g, p)
        F[k].data.copy_(torch.from_numpy(H[k]))
        F2[k].data.copy_(torch.from_numpy(H[k]))
    return g, H, F, F2


@pytest.mark.parametrize("with_obc", [False, True])
def test_python_wrapper_on_one_rank_is_the_single_domain_wrapper(D, with_obc):
    import torch
    g, H, F, F2 = _pygrid(D, 300, 70)
    prm = D.psy.momentum_params(*PRM)
    ssh_bc = 0.03125 if with_obc else None
    D.psy.invoke_nemolite_step(prm, *[F[k] for k in OUTS], *[F[k] for k in INS], ssh_bc=ssh_bc)
    D.psy.invoke_nemolite_step_dm(prm, *[F2[k] for k in OUTS], *[F2[k] for k in INS], ssh_bc=ssh_bc)
    torch.cuda.synchronize()
    for k in H:
        assert M.same(F2[k].get_data(), F[k].get_data()), k


def test_python_wrapper_refusals(D):
    """halo_width = 2: GoceanStop naming the halo width; no Coriolis parameter: GoceanStop; nothing is written"""
    import torch
    prm = D.psy.momentum_params(*PRM)
    g, H, F, _ = _pygrid(D, 64, 32, halo_width=2)
    with pytest.raises(D._cabi.GoceanStop, match="halo_width 2"):
        D.psy.invoke_nemolite_step_dm(prm, *[F[k] for k in OUTS], *[F[k] for k in INS])
    g1, H1, F1, _ = _pygrid(D, 64, 32, coriolis=False)
    with pytest.raises(D._cabi.GoceanStop, match="Coriolis"):
        D.psy.invoke_nemolite_step_dm(prm, *[F1[k] for k in OUTS], *[F1[k] for k in INS], ssh_bc=0.25)
    torch.cuda.synchronize()
    for k in OUTS:
        assert M.same(F[k].get_data(), H[k]) and M.same(F1[k].get_data(), H1[k]), k
