"""GPU test (-m gpu): the NEMOLite2D-class kernels on arrays of more than 2^31 ELEMENTS (46400^2 cells, 17.25 GB per f64
array), as tests/test_gpu_large_index.py does for Jacobi and shallow water: row bands cut out of the big arrays (at the start,
where the linear element index crosses 2^28 .. 2^31 -- for the int32 tmask its byte offset crosses 2^31 at 2^29 -- and at
the end) are swept again as SMALL arrays, the form tests/test_gpu_nemolite_subboxes.py pins to the CPU restatements, with the
same tuning key, and must equal the big sweep's rows.  Outputs the kernels write only in part start from the same contents:
their bands are copied before the big call; ssha of the row north of a band's box, which the band's last v faces read, is
the one the big sweep left there.  Read-only inputs share tensors (the refusals check outputs only) so that
everything fits: four f64 inputs, the int32 mask and five outputs, about 165 GB."""
import ctypes as C

import pytest

from nemolite_boxes import PRM

pytestmark = pytest.mark.gpu

N = 46400
LD = 46464            # DL_ESM_ALIGNMENT = 64: N + 2 padded
NY = N + 3
OUTS = ("ssha", "ssha_u", "ssha_v", "ua", "va")
SENT = -7.0


def _bands():
    """first rows of bands of five rows: the start, the rows where the linear element index crosses 2^28 (2^31 bytes), 2^29
    (2^31 bytes of tmask), 2^30, 2^31 elements, and the end"""
    rows = [0, NY - 5]
    for e in (28, 29, 30, 31):
        r = (1 << e) // LD
        rows += [r - 3, r - 1]
    return sorted(r for r in set(rows) if 0 <= r <= NY - 5)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def T():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    import dl_esm_inf_amd as d
    torch.cuda.set_device(0)
    d.parallel_init(0, 1)
    free, _ = torch.cuda.mem_get_info()
    if free < 200e9:
        pytest.skip(f"needs 200 GB of free device memory, {free / 1e9:.0f} GB there")
    g = torch.Generator(device="cuda")
    g.manual_seed(4321)

    def big(fn):
        t = torch.empty((NY, LD), dtype=torch.float64, device="cuda")
        for r0 in range(0, NY, 4096):            # (in slabs: the generator's temporaries stay small)
            t[r0:r0 + 4096].copy_(fn((min(4096, NY - r0), LD)))
        return t
    A = {"V": big(lambda s: 0.3 * torch.randn(s, dtype=torch.float64, device="cuda", generator=g)),
         "Hd": big(lambda s: 10.0 + torch.rand(s, dtype=torch.float64, device="cuda", generator=g)),
         "S": big(lambda s: 0.1 * torch.randn(s, dtype=torch.float64, device="cuda", generator=g)),
         "Mx": big(lambda s: 900.0 + 200.0 * torch.rand(s, dtype=torch.float64, device="cuda", generator=g))}
    tbl = torch.tensor([-1, 0, 1, 1, 1], dtype=torch.int32, device="cuda")
    tm = torch.empty((NY, LD), dtype=torch.int32, device="cuda")
    for r0 in range(0, NY, 4096):
        tm[r0:r0 + 4096].copy_(tbl[torch.randint(0, 5, (min(4096, NY - r0), LD), device="cuda", generator=g)])
    A["tmask"] = tm
    A["out"] = {k: torch.empty((NY, LD), dtype=torch.float64, device="cuda") for k in OUTS}
    torch.cuda.synchronize()
    yield torch, d, d._cabi.lib(), A, g
    A.clear()
    del tm
    torch.cuda.empty_cache()


def _reset(torch, A, g):
    """outputs: sentinels, ssha distinct values (its ring is read)"""
    for k, t in A["out"].items():
        if k == "ssha":
            for r0 in range(0, NY, 4096):
                t[r0:r0 + 4096].copy_(1000.0 + torch.rand((min(4096, NY - r0), LD), dtype=torch.float64, device="cuda",
                                                          generator=g))
        else:
            t.fill_(SENT)


def _grid(D, A, rows=None):
    """a dlesm_momentum_grid: every metric and area Mx, the Coriolis parameter V; on rows r..r+4 when rows = r"""
    cut = (lambda t: t) if rows is None else (lambda t: t[rows:rows + 5].contiguous())
    keep = {"tmask": cut(A["tmask"]), "Mx": cut(A["Mx"]), "V": cut(A["V"])}
    mx, v = keep["Mx"].data_ptr(), keep["V"].data_ptr()
    mg = D._cabi.MomentumGrid(tmask=keep["tmask"].data_ptr(), dx_t=mx, dy_t=mx, dx_u=mx, dy_u=mx, dx_v=mx, dy_v=mx,
                              area_u=mx, area_v=mx, fcor_u=v, fcor_v=v)
    return mg, keep


def _bands_then_compare(torch, D, A, names, run):
    """run(ld_ny_rows, inputs, outputs, grid) on the big arrays, then on every band as a small array from the band's
    pre-call contents; the band's rows inside the box must be equal, and the outputs' ring and padding keep their contents"""
    outs = A["out"]
    pre = {r: {k: outs[k][r:r + 5].clone() for k in names} for r in _bands()}
    edge = {k: (outs[k][:, 0].clone(), outs[k][:, N + 1:].clone()) for k in names}
    mg, keep = _grid(D, A)
    run(NY, (2, N + 1, 2, N + 1), {k: A[k] for k in ("V", "Hd", "S", "Mx")}, {k: outs[k] for k in names}, mg, keep)
    torch.cuda.synchronize()
    for r in _bands():
        lo, hi = max(r + 1, 1), min(r + 4, N + 1)         # rows of the big box among rows 2..4 (1-based) of the band
        mgs, ks = _grid(D, A, r)
        so = {k: pre[r][k].clone() for k in names}
        if "ssha" in names:
            # the row north of the small box: the v faces of its last row read ssha there -- in the big sweep the value it
            # computed (or, for the last band, the untouched ring row)
            so["ssha"][hi - r].copy_(outs["ssha"][hi])
        run(5, (2, N + 1, lo - r + 1, hi - r), {k: A[k][r:r + 5].contiguous() for k in ("V", "Hd", "S", "Mx")}, so, mgs, ks)
        torch.cuda.synchronize()
        for k in names:
            assert torch.equal(outs[k][lo:hi], so[k][lo - r:hi - r]), (r, k)
    for k in names:
        assert torch.equal(outs[k][0], pre[0][k][0]) and torch.equal(outs[k][N + 1:], pre[NY - 5][k][N + 1 - (NY - 5):]), k
        assert torch.equal(outs[k][:, 0], edge[k][0]) and torch.equal(outs[k][:, N + 1:], edge[k][1]), k
        if k != "ssha":
            assert bool((outs[k][1:N + 1, 1:N + 1] != SENT).any()), k


def _set_tuning(D, **kw):
    for k, v in kw.items():
        D._cabi.lib().dlesm_set_tuning(k.encode(), v)


def test_continuity_and_next_ssh_beyond_2_31_elements(T):
    torch, D, L, A, g = T
    assert LD * NY > 2 ** 31
    _reset(torch, A, g)

    def run(ny, box, I, O_, mg, keep):
        V, Hd, S, Mx = (_ptr(I[k]) for k in ("V", "Hd", "S", "Mx"))
        D._cabi.check(L.dlesm_continuity_f64(PRM[0], LD, ny, *box, S, S, S, Hd, Hd, V, V, Mx, _ptr(O_["ssha"]), None))
        tm = _ptr(keep["tmask"])
        D._cabi.check(L.dlesm_next_sshu_f64(LD, ny, *box, tm, Mx, Mx, S, _ptr(O_["ssha_u"]), None))
        D._cabi.check(L.dlesm_next_sshv_f64(LD, ny, *box, tm, Mx, Mx, S, _ptr(O_["ssha_v"]), None))
    _bands_then_compare(torch, D, A, ("ssha", "ssha_u", "ssha_v"), run)


@pytest.mark.parametrize("kernel", [0, 1])
def test_momentum_beyond_2_31_elements(T, kernel):
    """the fused entry, the tile (0) and the one-cell form (1); the bands with the same key"""
    torch, D, L, A, g = T
    _reset(torch, A, g)
    prm = D.psy.momentum_params(*PRM)

    def run(ny, box, I, O_, mg, keep):
        V, Hd, S = (_ptr(I[k]) for k in ("V", "Hd", "S"))
        r = D._cabi.Region(0, 0, *box)
        D._cabi.check(L.dlesm_momentum_f64(C.byref(prm), C.byref(mg), LD, ny, C.byref(r), C.byref(r),
                                           V, V, Hd, S, Hd, S, Hd, S, S, S, _ptr(O_["ua"]), _ptr(O_["va"]), None))
    try:
        _set_tuning(D, mom_kernel=kernel)
        _bands_then_compare(torch, D, A, ("ua", "va"), run)
    finally:
        _set_tuning(D, mom_kernel=0)


@pytest.mark.parametrize("kernel", [0, 1])
def test_nemolite_step_beyond_2_31_elements(T, kernel):
    """the one-call step on box (2, N+1, 2, N+1), no open-boundary plan: the tile (0) and the definition path (1)"""
    torch, D, L, A, g = T
    _reset(torch, A, g)
    prm = D.psy.momentum_params(*PRM)

    def run(ny, box, I, O_, mg, keep):
        V, Hd, S, Mx = (_ptr(I[k]) for k in ("V", "Hd", "S", "Mx"))
        r = D._cabi.Region(0, 0, *box)
        rc = L.dlesm_nemolite_step_f64(C.byref(prm), C.byref(mg), Mx, LD, ny, C.byref(r), C.byref(r), C.byref(r), None, 0.0,
                                       V, V, Hd, Hd, Hd, S, S, S, *[_ptr(O_[k]) for k in OUTS], None)
        assert rc == 0, L.dlesm_last_error()
    try:
        _set_tuning(D, nemo_step_kernel=kernel)
        _bands_then_compare(torch, D, A, OUTS, run)
    finally:
        _set_tuning(D, nemo_step_kernel=0)
