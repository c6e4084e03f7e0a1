"""GPU tests (-m gpu) of tracer transport on a decomposed grid, dlesm_tracer_step_dm, in loop-back on
one GPU: rank 0 is its own eight neighbours through depth-1 tables.  Each case compares the one call with its definition on
the same plan -- dlesm_tracer_step_f64, then dlesm_halo_exchange_multi_f64 of the new tracers -- over whole sentinel-filled
arrays, and with tests/tracer_numpy.py inside the box: over the RCCL group, and over mailboxes connected for three fields with
the RCCL group switched off underneath (dm_skip_parts = 1), with 1, 3 and 4 tracers, so that the exchange takes one turn and
two.  Also: a plan without messages is dlesm_tracer_step_f64; a depth-2 plan, a null plan and a plan of other extents are
refused; the Python wrappers."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

import oracle_lib as O
import tracer_cases as TC
import tracer_numpy as TN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))


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
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


class Case:
    """raw (ny, ld) device arrays on a box with a one-cell ring and a depth-1 loop-back plan.  The mask, the flow arrays and
    the tracers carry the periodic halos of the plan (the halos a neighbour would hold), computed on the host by the oracle's
    exchange; the outputs are sentinels"""

    def __init__(self, D, ld, ny, k, seed, shift=0, peer=0, tables=True):
        import torch
        from dm_overhead import loopback_tables
        self.D, self.L = D, D._cabi.lib()
        self.ld, self.ny, self.k = ld, ny, k
        self.box = (2, ld - 1, 2, ny - 1)
        rng = np.random.default_rng(seed)
        self.tm = TC.random_mask(rng, ny, ld)
        self.area_t, self.H = TC.flow_inputs(rng, self.tm)
        self.c_in, self.c_out = TC.tracers(rng, self.tm.shape, k)
        self.t = loopback_tables(D, D._cabi.Region(ld - 2, ny - 2, *self.box), 1) if tables else D._cabi.CommTables()
        if tables:
            oc = O.Comms()
            C.memmove(C.byref(oc), C.byref(self.t), C.sizeof(oc))
            tmf = self.tm.astype(np.float64)
            for a in [tmf, self.area_t] + list(self.H.values()) + self.c_in:
                assert O.exchange_all([a], [ld], [oc]) == 0
            self.tm = tmf.astype(np.int32)

        def dev(a):
            t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
            if shift:
                t = torch.cat([torch.zeros(1, dtype=t.dtype, device="cuda"), t.flatten()])[1:].view(a.shape)
            return t
        self.dev = dev
        self.I = {n: dev(a) for n, a in self.H.items()}
        self.area = dev(self.area_t)
        self.tmd = torch.from_numpy(self.tm).cuda()
        self.ci = [dev(a) for a in self.c_in]
        self.plan = C.c_void_p()
        D._cabi.check(self.L.dlesm_halo_plan_create(C.byref(self.t), ld, ny, C.byref(self.plan)))
        self.peer = peer
        if peer:
            from dl_esm_inf_amd import grid_mod
            grid_mod.connect_peers(types.SimpleNamespace(_halo_plan=self.plan), peer)
            self.L.dlesm_set_tuning(b"dm_skip_parts", 1)      # no RCCL group: only the mailboxes can move the halos

    def outputs(self):
        return [self.dev(a) for a in self.c_out]

    def flow(self):
        return [_p(self.tmd), _p(self.area)] + [_p(self.I[n]) for n in TC.FLOW]

    def single(self, co):
        return self.L.dlesm_tracer_step_f64(TC.RDT, self.ld, self.ny, *self.box, *self.flow(), _ptrs(self.ci), _ptrs(co),
                                            self.k, None)

    def one_call(self, co, plan=None):
        return self.L.dlesm_tracer_step_dm(self.plan if plan is None else plan, TC.RDT, self.ld, self.ny, *self.box,
                                           *self.flow(), _ptrs(self.ci), _ptrs(co), self.k, None)

    def close(self):
        self.L.dlesm_set_tuning(b"dm_skip_parts", 0)
        self.L.dlesm_set_tuning(b"tracer_kernel", 0)
        self.D._cabi.check(self.L.dlesm_halo_plan_destroy(self.plan))


@pytest.mark.parametrize("peer", [0, 3])
@pytest.mark.parametrize("k", [1, 3, 4])
@pytest.mark.parametrize("ld,ny,shift,kernel", [
    (300, 70, 0, 0),     # even pitch, aligned: the tile
    (301, 41, 0, 0),     # odd pitch: the general path
    (256, 33, 1, 0),     # bases 8 bytes off a 16-byte boundary
    (130, 21, 0, 1),     # the HOOK key tracer_kernel = 1
    (6, 5, 0, 0),        # a 4 x 3 box
])
def test_one_call_equals_the_definition(D, ld, ny, shift, kernel, k, peer):
    """whole sentinel-filled arrays: every cell of every new tracer equals step + exchange, inputs untouched; peer = 3: the
    mailboxes connected for three fields (four tracers: two turns), the RCCL group switched off"""
    import torch
    S = Case(D, ld, ny, k, ld * 31 + ny + shift + k, shift=shift, peer=peer)
    try:
        S.L.dlesm_set_tuning(b"tracer_kernel", kernel)
        Od, O1 = S.outputs(), S.outputs()
        assert S.single(Od) == 0, S.L.dlesm_last_error()
        # (with the RCCL group off an exchange of more fields than the mailboxes hold moves nothing: the definition takes the
        #  turns dlesm_halo_exchange_multi_f64 takes in mailbox mode)
        turn = peer or k
        for n in range(0, k, turn):
            D._cabi.check(S.L.dlesm_halo_exchange_multi_f64(S.plan, _ptrs(Od[n:n + turn]), len(Od[n:n + turn]),
                                                            D._cabi.DIRS_ALL, None))
        assert S.one_call(O1) == 0, S.L.dlesm_last_error()
        torch.cuda.synchronize()
        assert S.L.dlesm_wait_timed_out(0) == 0
        want = TC.reference(TC.RDT, S.box, S.tm, S.area_t, S.H, S.c_in, S.c_out)
        for n in range(k):
            got, dfn = O1[n].cpu().numpy(), Od[n].cpu().numpy()
            assert TN.same(got, dfn), (n, np.argwhere(got != dfn)[:5])
            assert TN.same(got[1:-1, 1:-1], want[n][1:-1, 1:-1]), n
            # the halos moved: the east halo column holds the west internal column (loop-back), the north row the south one
            assert TN.same(got[1:-1, ld - 1], got[1:-1, 1]) and TN.same(got[ny - 1, 1:-1], got[1, 1:-1])
            assert TN.same(S.ci[n].cpu().numpy(), S.c_in[n])
        for n in TC.FLOW:
            assert TN.same(S.I[n].cpu().numpy(), S.H[n]), n
    finally:
        S.close()


@pytest.mark.parametrize("k", [1, 5])
def test_plan_without_messages_is_the_single_domain_call(D, k):
    import torch
    S = Case(D, 300, 70, k, 4242, tables=False)
    try:
        Os, O1 = S.outputs(), S.outputs()
        assert S.single(Os) == 0 and S.one_call(O1) == 0, S.L.dlesm_last_error()
        torch.cuda.synchronize()
        for n in range(k):
            assert TN.same(O1[n].cpu().numpy(), Os[n].cpu().numpy()), n
            assert (O1[n].cpu().numpy() != TC.SENTINEL).any()
    finally:
        S.close()


def test_refusals(D):
    """a depth-2 plan with messages, a null plan, a plan of other extents, and the single-domain entry's refusals through the
    distributed one: DLESM_EINVAL before anything is launched or exchanged -- every array untouched"""
    import torch
    from dm_overhead import loopback_tables
    S = Case(D, 64, 24, 2, 5)
    L = S.L
    t2 = loopback_tables(D, D._cabi.Region(60, 20, 3, 62, 3, 22), 2)
    plan2, plan3 = C.c_void_p(), C.c_void_p()
    D._cabi.check(L.dlesm_halo_plan_create(C.byref(t2), 64, 24, C.byref(plan2)))
    D._cabi.check(L.dlesm_halo_plan_create(C.byref(S.t), 66, 24, C.byref(plan3)))
    try:
        co = S.outputs()
        got = []
        for plan, msg in ((plan2, b"depth-2"), (C.c_void_p(0), b"null plan"), (plan3, b"66x24")):
            rc = S.one_call(co, plan=plan)
            got.append((rc, msg in L.dlesm_last_error(), L.dlesm_last_error()))
        rc = S.one_call([co[0], co[0]])
        got.append((rc, b"overlap" in L.dlesm_last_error(), L.dlesm_last_error()))
        rc = S.one_call([S.ci[1], co[1]])
        got.append((rc, b"overlaps c_in[1]" in L.dlesm_last_error(), L.dlesm_last_error()))
        S.k = 9
        rc = S.one_call(co)
        S.k = 2
        got.append((rc, b"9 tracers" in L.dlesm_last_error(), L.dlesm_last_error()))
        assert all(rc == D._cabi.EINVAL and ok for rc, ok, _ in got), got
        torch.cuda.synchronize()
        for n in range(2):
            assert (co[n].cpu().numpy() == TC.SENTINEL).all() and TN.same(S.ci[n].cpu().numpy(), S.c_in[n])
    finally:
        S.close()
        L.dlesm_halo_plan_destroy(plan2)
        L.dlesm_halo_plan_destroy(plan3)


def _pygrid(D, nx, ny, halo_width=1):
    import torch
    os.environ["DL_ESM_ALIGNMENT"] = "64"
    try:
        g = D.grid_type(D.GO_ARAKAWA_C, (1, 1, 2), D.GO_OFFSET_NE)
        g.decompose(nx, ny, halo_width=halo_width)
        rng = np.random.default_rng(nx + ny)
        user = TC.random_mask(rng, ny + 2, nx + 2)
        D.grid_init(g, 1000.0, 1000.0, tmask=user if halo_width == 1 else None)
    finally:
        os.environ.pop("DL_ESM_ALIGNMENT", None)
    T, U, V = D.GO_T_POINTS, D.GO_U_POINTS, D.GO_V_POINTS
    pts = {"ssha": T, "sshn_t": T, "ht": T, "sshn_u": U, "un": U, "hu": U, "sshn_v": V, "vn": V, "hv": V}
    H = {n: (10.0 + rng.random((g.ny, g.nx)) if n in ("ht", "hu", "hv") else 0.1 * rng.normal(size=(g.ny, g.nx))) for n in pts}
    F = {}
    for n, p in pts.items():
        F[n] = D.r2d_field(g, p)
        F[n].data.copy_(torch.from_numpy(H[n]))
    c = [1.0 + n + rng.random((g.ny, g.nx)) for n in range(3)]

    def tracers(arrays):
        out = []
        for a in arrays:
            f = D.r2d_field(g, T)
            f.data.copy_(torch.from_numpy(a))
            out.append(f)
        return out
    return g, F, c, tracers


def _order(F):
    return [F[n] for n in ("ssha", "un", "vn", "ht", "hu", "hv", "sshn_t", "sshn_u", "sshn_v")]


def test_python_wrapper_on_one_rank_is_the_single_domain_wrapper(D):
    import torch
    g, F, c, tracers = _pygrid(D, 300, 70)
    Ci = tracers(c)
    Co1, Co2 = tracers([np.full_like(a, TC.SENTINEL) for a in c]), tracers([np.full_like(a, TC.SENTINEL) for a in c])
    D.psy.invoke_tracer_step(TC.RDT, Co1, Ci, *_order(F))
    D.psy.invoke_tracer_step_dm(TC.RDT, Co2, Ci, *_order(F))
    torch.cuda.synchronize()
    for n in range(3):
        assert TN.same(Co2[n].get_data(), Co1[n].get_data()), n
        assert (Co1[n].get_data() != TC.SENTINEL).any()


def test_python_wrapper_refuses_another_halo_width(D):
    import torch
    g, F, c, tracers = _pygrid(D, 64, 32, halo_width=2)
    Ci, Co = tracers(c), tracers([np.full_like(a, TC.SENTINEL) for a in c])
    with pytest.raises(D._cabi.GoceanStop, match="halo_width 2"):
        D.psy.invoke_tracer_step_dm(TC.RDT, Co, Ci, *_order(F))
    torch.cuda.synchronize()
    assert all((f.get_data() == TC.SENTINEL).all() for f in Co)
