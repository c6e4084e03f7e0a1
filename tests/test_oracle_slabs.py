"""The slab-parallel form of the oracle (oracle_lib.slabs and its *_slabs entries) -- what the full-size GPU tests compare
whole fields with -- equals one whole-array call of the same single-threaded entry, bit for bit, every cell of every output:
odd and even leading dimensions, band counts that do not divide the height, one band, and more bands than rows."""
import functools

import numpy as np
import pytest

import oracle_lib as O

SHAPES = [(23, 37), (23, 40), (4, 9)]          # (ny, ld): odd and even ld; a box of two rows
BANDS = [(5, 3), (1, 1), (7, 4), (64, 2)]      # (bands, threads): 21 rows in 5 / 7 bands, one band, more bands than rows
PRM = O.SwParams(4.0 / 1.0e5, 4.0 / 0.9e5, 80.0 / 8.0, 80.0 / 1.0e5, 80.0 / 0.9e5)


def _fields(ny, ld, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.random((ny, ld)) * 0.2 + (1.0 if k % 3 == 2 else -0.1) for k in range(n)]


def _box(ny, ld, ring=1):
    return (1 + ring, ld - ring, 1 + ring, ny - ring)


def _same(a, b, what):
    assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), (what, np.argwhere(a != b)[:4].tolist())


def _outs(ny, ld, n):
    """n sentinel-filled output arrays"""
    return [np.full((ny, ld), -7.0) for _ in range(n)]


def _split(monkeypatch, bands, threads):
    """every *_slabs entry with `bands` bands on `threads` threads"""
    monkeypatch.setattr(O, "slabs", functools.partial(O.slabs, bands=bands, threads=threads))


@pytest.mark.parametrize("bands,threads", BANDS)
@pytest.mark.parametrize("ny,ld", SHAPES)
def test_stencils_by_slabs_equal_one_call(ny, ld, bands, threads, monkeypatch):
    _split(monkeypatch, bands, threads)
    box = _box(ny, ld)
    (inp,) = _fields(ny, ld, 1, ny * ld)
    tmask = np.random.default_rng(3).integers(-1, 2, (ny, ld)).astype(np.int32)
    coef = np.random.default_rng(4).random(9) - 0.45
    cases = [("jacobi5", O.jacobi5, O.jacobi5_slabs, [inp]),
             ("jacobi5_masked", O.jacobi5_masked, O.jacobi5_masked_slabs, [inp, None, tmask]),
             ("stencil9", O.stencil9, O.stencil9_slabs, [inp, None, coef])]
    for name, whole, by_slabs, args in cases:
        want, got = _outs(ny, ld, 2)
        whole(*args[:1], want, *args[2:], ld, *box)
        by_slabs(*args[:1], got, *args[2:], ld, *box)
        _same(got, want, name)
    ins = _fields(ny, ld, 8, ny + ld)
    ins[7] += 0.5                                           # area_t
    want, got = _outs(ny, ld, 2)
    O.continuity(0.37, ld, box, *ins, want)
    O.continuity_slabs(0.37, ld, box, *ins, got)
    _same(got, want, "continuity")


@pytest.mark.parametrize("bands,threads", BANDS)
@pytest.mark.parametrize("ny,ld", SHAPES)
@pytest.mark.parametrize("sw_offset", [False, True], ids=["NE", "SW"])
def test_shallow_by_slabs_equals_one_call(ny, ld, bands, threads, sw_offset, monkeypatch):
    _split(monkeypatch, bands, threads)
    box = _box(ny, ld)
    ins = _fields(ny, ld, 6, 7 * ny + ld)
    want, got = _outs(ny, ld, 3), _outs(ny, ld, 3)
    (O.sw_step_sw if sw_offset else O.sw_step)(PRM, ld, box, *ins, *want)
    (O.sw_step_sw_slabs if sw_offset else O.sw_step_slabs)(PRM, ld, box, *ins, *got)
    for k in range(3):
        _same(got[k], want[k], ("step", k))
    # the eight GOcean kernels one by one, each a loop nest of its own; time_smooth reads its output (field_old) too
    arity = dict(cu=2, cv=2, z=3, h=3, unew=4, vnew=4, pnew=3, time_smooth=2)
    for name in O.SW_KERNELS:
        a = _fields(ny, ld, arity[name], len(name) * 31 + ny)
        want, got = _fields(ny, ld, 1, 5)[0], _fields(ny, ld, 1, 5)[0]
        s0, s1 = 0.37, -1.25
        O.sw_kernel(name, sw_offset, ld, box, want, a + ([want] if name == "time_smooth" else []), s0, s1)
        O.sw_kernel_slabs(name, sw_offset, ld, box, got, a + ([got] if name == "time_smooth" else []), s0, s1)
        _same(got, want, name)
