"""Inputs the CPU and GPU tests of the cell bin share, made once and never modified: the particles
are those of tests/particle_order_cases.py, the order is its reference, and every particle gets two weights whose magnitudes
are mixed -- a sign, one of 2^60, 1 and 2^-30, and a random mantissa -- so that the bits of a sum depend on the order in which
it was added.  Nothing here needs a GPU."""
import numpy as np

import cell_bin_numpy as BN
import particle_order_cases as PC

NS = [1, 63, 64, 65, 128, 129, 257, 4097, 70001]
BOXNAMES = ["empty", "1x1", "15x16", "256x256"]
_MADE = {}


def weights(n, which):
    """weight array `which` (1 or 2) of n particles"""
    key = ("w", n, which)
    if key not in _MADE:
        rng = np.random.default_rng(619000 + 7 * n + which)
        scale = rng.choice(np.array([2.0 ** 60, 1.0, 2.0 ** -30]), n)
        sign = rng.choice(np.array([-1.0, 1.0]), n)
        w = sign * scale * (1.0 + rng.random(n))
        w.setflags(write=False)
        _MADE[key] = w
    return _MADE[key]


def reference(dist, boxname, n):
    """(S, has) of a case in its reference order, by the array restatement: rows count, weights 1, weights 2; made once"""
    key = ("ref", dist, boxname, n)
    if key not in _MADE:
        perm = PC.reference(dist, boxname, n)[0]
        S, has, unordered = BN.sums_array(PC.BOXES[boxname], *PC.case(dist, boxname, n), perm, [None, weights(n, 1), weights(n, 2)])
        assert unordered == 0
        S.setflags(write=False), has.setflags(write=False)
        _MADE[key] = (S, has)
    return _MADE[key]
