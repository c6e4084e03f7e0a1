"""Inputs the CPU and GPU tests of the dispersal step share, made once and never modified: the grid,
the flow and the particle pool are those of tests/drifter_cases.py; here are the diffusivity, the seed, the tick, the
identities and the references by the restatements of tests/dispersal_numpy.py.  Nothing here needs a GPU.

KH = 37.5 m2/s with H = 400 s gives an amplitude sqrt(6 KH H) of exactly 300 m, about a third of a cell.  The seed's high
word is not zero, and TICK = 2^32 - 2 with nsub = 3 carries from the low into the high counter word.
"""
import numpy as np

import dispersal_numpy as PN
import drifter_cases as DC

KH = 37.5
SEED = 0xC0FFEE1234567891           # as a signed 64-bit number it is negative
TICK = 2 ** 32 - 2
_MADE = {}


def signed(seed):
    """the seed as the C ABI's long long"""
    seed &= PN.MASK64
    return seed - (1 << 64) if seed >> 63 else seed


def ids():
    """one int32 identity per particle of the pool: random over all 32 bits, negative ones among them, every seventh a
    duplicate of its neighbour"""
    if "ids" not in _MADE:
        rng = np.random.default_rng(6200)
        a = rng.integers(-2 ** 31, 2 ** 31, DC.POOL).astype(np.int32)
        a[1::7] = a[0:-1:7][:len(a[1::7])]
        a[0], a[2] = -1, -2 ** 31
        _MADE["ids"] = a
    return _MADE["ids"]


def reference(box, nsub, with_ids, kh=KH, seed=SEED, tick=TICK, calls=1):
    """the pool after `calls` calls (the tick advanced by nsub between them) by the array restatement; made once.  Returns
    (px, py, status, census)"""
    key = ("ref", tuple(box), nsub, with_ids, kh, seed, tick, calls)
    if key not in _MADE:
        px, py, st = (a.copy() for a in DC.particles())
        seen = {}
        for c in range(calls):
            PN.dispersal_step(DC.H, nsub, kh, seed, tick + c * nsub, box, *DC.flow(), px, py, st,
                              ids() if with_ids else None, seen)
        _MADE[key] = (px, py, st, seen)
    return _MADE[key]


def scalar_reference(box, nsub, with_ids, kh=KH, seed=SEED, tick=TICK):
    """the first NSCALAR particles after one call by the scalar restatement; made once"""
    key = ("scalar", tuple(box), nsub, with_ids, kh, seed, tick)
    if key not in _MADE:
        px, py, st = (a[:DC.NSCALAR].copy() for a in DC.particles())
        seen = {}
        PN.dispersal_step_scalar(DC.H, nsub, kh, seed, tick, box, *DC.flow(), px, py, st,
                                 ids()[:DC.NSCALAR] if with_ids else None, seen)
        _MADE[key] = (px, py, st, seen)
    return _MADE[key]
