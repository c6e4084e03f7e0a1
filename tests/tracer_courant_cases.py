"""Inputs the CPU and GPU tests of the tracer schemes' Courant check share: the plain and the
special-value case of tracer_cases at its three shapes, the land overwrite of the invariance tests, the cells of
special_case's patch whose largest face number is exactly 1 and one ulp below, and the restatement's record of each, made
once and never modified.  Nothing here needs a GPU.
"""
import numpy as np

import tracer_cases as TC
import tracer_courant_numpy as CN

ARRAYS = ("un", "vn", "hu", "hv", "ht", "sshn_t", "sshn_u", "sshn_v")      # the C entry's order, after tmask and area_t
LIMITS = (0.5, 1.0)
_MADE = {}


def plain_host(ld, ny):
    """(tm, area_t, H): random_mask + flow_inputs with the modules' seeding rule"""
    key = ("plain", ld, ny)
    if key not in _MADE:
        rng = np.random.default_rng(ld * 7 + ny)
        tm = TC.random_mask(rng, ny, ld)
        area_t, H = TC.flow_inputs(rng, tm)
        _MADE[key] = (tm, area_t, H)
    return _MADE[key]


def special_host(ld, ny, rdt):
    tm, area_t, H, _, _ = TC.special_host(ld, ny, rdt)
    return tm, area_t, H


def host(kind, ld, ny, rdt):
    return plain_host(ld, ny) if kind == "plain" else special_host(ld, ny, rdt)


def flow(H):
    return [H[k] for k in ARRAYS]


def reference(kind, ld, ny, box, rdt, limits=LIMITS):
    """the array restatement's record of the case; made once"""
    key = (kind, ld, ny, tuple(box), float(rdt), tuple(limits))
    if key not in _MADE:
        tm, area_t, H = host(kind, ld, ny, rdt)
        _MADE[key] = CN.tracer_courant(rdt, box, tm, area_t, *flow(H), *limits)
    return _MADE[key]


def land_overwritten(tm, area_t, H):
    """copies with NaN in un / vn on every face that touches land (tracer_cases.overwrite_land) and in area_t, ht and
    sshn_t on every land cell"""
    H2, _ = TC.overwrite_land(tm, H, [], np.nan)
    a2 = area_t.copy()
    a2[tm == 0] = np.nan
    for k in ("ht", "sshn_t"):
        H2[k][tm == 0] = np.nan
    return a2, H2


PROBE = (21, 5)                                    # 1-based (i, j) of a cell of special_case's PATCH with patch cells all round


def patch_probe(H, top):
    """a copy of the flow in which PROBE's four face velocities are top, 0.5, -0.0 and -ONE_BELOW: the patch has unit
    weights, so the cell's face numbers are 1-ulp, 0.5, 0 and `top` exactly"""
    i, j = PROBE[0] - 1, PROBE[1] - 1
    rows, cols = TC.PATCH
    assert rows.start < j < rows.stop - 1 and cols.start < i < cols.stop - 2
    H2 = {k: v.copy() for k, v in H.items()}
    H2["un"][j, i], H2["un"][j, i - 1], H2["vn"][j, i], H2["vn"][j - 1, i] = -TC.ONE_BELOW, 0.5, -0.0, top
    return H2
