"""CPU test of the assumption land skipping rests on: no written cell of a NEMOLite2D-class time loop
ever consumes the ssha or sshn_t of a land cell (T == 0).  A skipped tile leaves its land ssha as it was, callers rotate ssha
into sshn_t, so stale land values travel through the loop; they must reach nothing.

Two runs of six tidal steps from the same state with the restatements of tests/ (the continuity oracle, momentum_numpy,
open_bc_numpy) in the order continuity -> next_sshu / next_sshv -> momentum -> bc_open, rotating by reference.  In the second
run every T == 0 cell of sshn_t and ssha is overwritten, before and after continuity of every step, with values drawn from
{NaN, 1e300, -3, 0}.  ssha_u, ssha_v, ua and va must hold the same bits in every cell after every step, ssha wherever T != 0.
It passes on the present kernels; it is there to fail if a later change of the specification makes a land value reach a
written cell."""
import numpy as np
import pytest

import momentum_numpy as M
import nemolite_boxes as NB
import open_bc_numpy as B
import oracle_lib as O

LD, NY, STEPS = 300, 40, 6
BOX = (2, LD - 1, 2, NY - 1)
POISON = np.array([np.nan, 1e300, -3.0, 0.0])
ROTATE = (("un", "ua"), ("vn", "va"), ("sshn_t", "ssha"), ("sshn_u", "ssha_u"), ("sshn_v", "ssha_v"))


def _mask(rng):
    """random -1/0/1 with land blocks, repaired for the open-boundary restatements: more than half land"""
    tm = rng.choice(np.array([-1, 0, 1, 1, 1], dtype=np.int32), size=(NY, LD))
    for _ in range(14):
        j, i = int(rng.integers(0, NY - 4)), int(rng.integers(0, LD - 30))
        tm[j:j + int(rng.integers(4, 16)), i:i + int(rng.integers(20, 70))] = 0
    return B.repair(tm)


def _run(seed, poison):
    rng = np.random.default_rng(seed)
    tm = _mask(rng)
    G = M.SimpleNamespace(**NB.host_grid(rng, tm))
    H = {**NB._host_inputs(rng, (NY, LD)), **NB._host_outputs(rng, (NY, LD))}
    hp = M.params(*NB.PRM)
    land = tm == 0
    prng = np.random.default_rng(seed + 1000)

    def spoil():
        if poison:
            for k in ("sshn_t", "ssha"):
                H[k][land] = prng.choice(POISON, size=int(land.sum()))

    trace = []
    for step in range(STEPS):
        ssh_bc = B.tide(0.1, 2.0 * np.pi / 43200.0, (step + 1) * NB.PRM[0])
        spoil()
        O.continuity(NB.PRM[0], LD, BOX, H["sshn_t"], H["sshn_u"], H["sshn_v"], H["hu"], H["hv"], H["un"], H["vn"], G.area_t,
                     H["ssha"])
        spoil()
        M.next_sshu(BOX, tm, G.area_t, G.area_u, H["ssha"], H["ssha_u"])
        M.next_sshv(BOX, tm, G.area_t, G.area_v, H["ssha"], H["ssha_v"])
        M.momentum(hp, G, BOX, BOX, *[H[k] for k in NB.MOM], H["ua"], H["va"])
        B.bc_open(hp, BOX, BOX, BOX, tm, ssh_bc, H["hu"], H["sshn_u"], H["hv"], H["sshn_v"], H["sshn_t"], H["ssha"], H["ua"],
                  H["va"])
        trace.append({k: H[k].copy() for k in NB.OUTS})
        for a, b in ROTATE:
            H[a], H[b] = H[b], H[a]
    return tm, trace


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_land_ssh_reaches_no_written_cell(seed):
    tm, clean = _run(seed, False)
    tm2, dirty = _run(seed, True)
    assert np.array_equal(tm, tm2)
    assert float((tm == 0).mean()) > 0.5 and (tm < 0).any() and (tm > 0).any()
    wet = tm != 0
    for step, (a, b) in enumerate(zip(clean, dirty)):
        for k in NB.OUTS[1:]:
            assert M.same(a[k], b[k]), (step, k)
        assert M.same(a["ssha"][wet], b["ssha"][wet]), step
    # the run did something, and the poison was in place: land ssha differs
    assert (clean[-1]["ua"] != -7.0).any() and (clean[-1]["va"] != -7.0).any()
    assert not M.same(clean[-1]["ssha"], dirty[-1]["ssha"])
