"""CPU tests of tests/nemolite_boxes.py: the box generator keeps the ring and reaches every edge placement of the two wave
tiles, and on its boxes -- and on the IEEE special-value inputs -- the vectorised restatements of momentum_numpy and
open_bc_numpy equal their scalar twins on every cell."""
import numpy as np
import pytest

import momentum_numpy as M
import nemolite_boxes as NB
import open_bc_numpy as B

CASES = NB.cases()


def _required(width):
    need = {("parity", a, b) for a in (0, 1) for b in (0, 1)}
    need |= {("last_lane", r % width) for r in (width - 3, width - 2, width - 1, width, width + 1)}
    need |= {("first_offset", d) for d in (0, 1, 7)} | {("first_wave", 1), ("first_wave", 2)}
    need |= {("spans_wave", 1), ("spans_wave", 2), ("cols", 1), ("cols", 2), ("one_col_odd",), ("rows", 1), ("rows", 2),
             ("ys2",), ("ye_last",), ("ring", "small"), ("ring", "large"), ("empty", "u"), ("empty", "v"),
             ("empty", "all"), ("uv_differ_every_edge",), ("uv_overlap",)}
    return need


def test_cases_are_deterministic_and_keep_the_ring():
    assert CASES == NB.cases() and len(CASES) >= NB.N_FIXED + 60
    for c in CASES:
        assert c.ny >= 3 and c.ld >= 8
        for b in (c.tbox, c.ubox, c.vbox):
            if not NB.empty(b):
                assert 2 <= b[0] <= b[1] <= c.ld - 1 and 2 <= b[2] <= b[3] <= c.ny - 1, c


@pytest.mark.parametrize("width", NB.WIDTHS)
def test_fixed_cases_reach_every_edge_placement(width):
    """every class of edge placement, for both tile widths, on cases the tiles take (even ld, aligned bases)"""
    fixed = CASES[:NB.N_FIXED]
    assert all(NB.tile_case(c) for c in fixed)
    got = set()
    for c in fixed:
        got |= NB.classes(c, width)
    assert not _required(width) - got, sorted(_required(width) - got)


def test_random_cases_mix_the_paths():
    rnd = CASES[NB.N_FIXED:]
    assert sum(c.ld % 2 for c in rnd) >= 5 and sum(c.shift for c in rnd) >= 4
    assert sum(NB.tile_case(c) and c.tbox == c.ubox == c.vbox for c in rnd) >= 20
    assert max(c.ld for c in rnd) >= 1000 and min(c.ny for c in rnd) <= 5


def _compare(case, seed, special=False):
    ld, ny, tbox, ubox, vbox, _ = case
    if special:
        tm, Gd, H, _ = NB.special_inputs(seed, ld, ny)
    else:
        rng = np.random.default_rng(seed)
        tm = NB.mask(rng, ny, ld)
        Gd = NB.host_grid(rng, tm)
        H = NB._host_inputs(rng, (ny, ld))
        H["ssha_u"] = 0.1 * rng.normal(size=(ny, ld))
        H["ssha_v"] = 0.1 * rng.normal(size=(ny, ld))
    G = M.SimpleNamespace(**Gd)
    hp = M.params(*NB.PRM)
    ins = [H[k] for k in NB.MOM]
    for vec, sca, box, last in ((M.momentum_u, M.momentum_u_scalar, ubox, H["ssha_u"]),
                                (M.momentum_v, M.momentum_v_scalar, vbox, H["ssha_v"])):
        a, b = np.full((ny, ld), -7.0), np.full((ny, ld), -7.0)
        vec(hp, G, box, *ins[:8], last, a)
        sca(hp, G, box, *ins[:8], last, b)
        assert M.same(a, b), vec.__name__
    for vec, sca, box, area in ((M.next_sshu, M.next_sshu_scalar, ubox, G.area_u), (M.next_sshv, M.next_sshv_scalar, vbox,
                                                                                    G.area_v)):
        a, b = np.full((ny, ld), -7.0), np.full((ny, ld), -7.0)
        vec(box, tm, G.area_t, area, H["sshn_t"], a)
        sca(box, tm, G.area_t, area, H["sshn_t"], b)
        assert M.same(a, b), vec.__name__
    a, b = H["sshn_t"].copy(), H["sshn_t"].copy()
    B.bc_ssh(tbox, tm, 0.0625, a)
    B.bc_ssh_scalar(tbox, tm, 0.0625, b)
    assert M.same(a, b)
    for vec, sca, box, h, s in ((B.flather_u, B.flather_u_scalar, ubox, "hu", "sshn_u"),
                                (B.flather_v, B.flather_v_scalar, vbox, "hv", "sshn_v")):
        a, b = H["un"].copy(), H["un"].copy()
        vec(hp, box, tm, H[h], H[s], H["sshn_t"], a)
        sca(hp, box, tm, H[h], H[s], H["sshn_t"], b)
        assert M.same(a, b), vec.__name__


# the scalar loops are slow: every fixed case of at most ~300 columns, and a sample of the random ones
SAMPLE = [k for k, c in enumerate(CASES) if (k < NB.N_FIXED and c.ld <= 300) or (k >= NB.N_FIXED and k % 6 == 0)]


@pytest.mark.parametrize("k", SAMPLE, ids=[NB.case_id(k, CASES[k]) for k in SAMPLE])
def test_vectorised_equals_scalar_on_the_generated_boxes(k):
    _compare(CASES[k], 1000 + k)


@pytest.mark.parametrize("ld,ny,box", [(256, 12, (2, 255, 2, 11)), (130, 9, (5, 100, 3, 8)), (129, 10, (2, 128, 2, 9))])
def test_vectorised_equals_scalar_on_special_values(ld, ny, box):
    """the special-value inputs of the GPU tests: the two restatements agree, and the results hold infinities, NaN and
    subnormals"""
    _compare(NB.Case(ld, ny, box, box, box, 0), ld * 3 + ny, special=True)
    tm, Gd, H, _ = NB.special_inputs(ld * 3 + ny, ld, ny)
    u, v = np.full((ny, ld), -7.0), np.full((ny, ld), -7.0)
    M.momentum(M.params(*NB.PRM), M.SimpleNamespace(**Gd), box, box, *[H[k] for k in NB.MOM], u, v)
    w = np.concatenate([u[u != -7.0], v[v != -7.0]])
    assert np.isinf(w).any() and np.isnan(w).any() and NB.is_subnormal(w).any()
