"""GPU test (-m gpu) that pins what the six NEMOLite2D distributed entries refuse, and in which order: dlesm_nemolite_step_dm,
dlesm_nemolite_step_wet_dm, dlesm_tracer_step_dm, dlesm_tracer_step_muscl_dm, dlesm_tracer_step_hancock_dm and
dlesm_nemolite_coupled_step_dm share one body, and every refusal of that body keeps its return code,
its place among the refusals and its WHOLE text, with the entry's own name in front.  One process, loop-back on one GPU, the
cases of tests/test_gpu_coupled_step_dm.py: 64 x 24 arrays with the box (2:63, 2:23) on a depth-1 plan and the box (3:62, 3:22)
on a depth-2 plan, a depth-3 plan, a plan made for 66 x 24 arrays.  Nothing is launched: after all the calls every output
still holds its sentinel and every input its values.  The texts are literals written from the format strings."""
import ctypes as C

import pytest

import momentum_numpy as M
import tracer_cases as TC
from test_gpu_coupled_step_dm import INS, OUTS, PRM, Case, D, _p, _ptrs, _R, one_call  # noqa: F401  (D: the fixture)

pytestmark = pytest.mark.gpu

FLOW_ENTRIES = ("dlesm_nemolite_step_dm", "dlesm_nemolite_step_wet_dm")
TRACER_ENTRIES = {"dlesm_tracer_step_dm": 1, "dlesm_tracer_step_muscl_dm": 2, "dlesm_tracer_step_hancock_dm": 2}   # depth
COUPLED = "dlesm_nemolite_coupled_step_dm"

NULL_PLAN = "%s: null plan"
EXTENTS = "%s: the plan is for 66x24 fields, got 64x24"
DEPTH = "%s: the plan exchanges depth-%d halos, the step needs depth %d (a grid decomposed with halo_width = %d)"
DEPTH_1_OR_2 = "%s: the plan exchanges depth-3 halos, the step needs depth 1 or 2 (a grid decomposed with halo_width = 1 or 2)"
LIMITED = ("%s: the plan exchanges depth-1 halos, the limited tracer schemes need depth 2 (a grid decomposed with "
           "halo_width = 2)")
ONE_BOX = ("%s: on a decomposed grid the T, U and V boxes must be one box (every NE grid): T (%d:%d,%d:%d), U (%d:%d,%d:%d), "
           "V (%d:%d,%d:%d)")


def _flow(S, entry, O_, prm, plan=None, boxes=None):
    tb, ub, vb = boxes or (S.box,) * 3
    wet = (None,) if entry.endswith("_wet_dm") else ()
    return getattr(S.L, entry)(S.plan if plan is None else plan, *wet, C.byref(prm), C.byref(S.mg), _p(S.gdev["area_t"]), S.ld,
                               S.ny, _R(S.D, tb), _R(S.D, ub), _R(S.D, vb), None, 0.0, *[_p(S.I[n]) for n in INS],
                               *[_p(O_[n]) for n in OUTS], None)


def _tracers(S, entry, O_, co, plan=None, ci=None, k=None):
    flow = {**S.I, "ssha": O_["ssha"]}
    ci = S.ci if ci is None else ci
    return getattr(S.L, entry)(S.plan if plan is None else plan, TC.RDT, S.ld, S.ny, *S.box, _p(S.gdev["tmask"]),
                               _p(S.gdev["area_t"]), *[_p(flow[n]) for n in TC.FLOW], _ptrs(ci), _ptrs(co),
                               len(co) if k is None else k, None)


def test_every_refusal_keeps_its_code_its_place_and_its_text(D):
    import torch
    from dm_overhead import loopback_tables
    S1, S2 = Case(D, 64, 24, 1, 2, 11), Case(D, 64, 24, 2, 2, 12)
    assert S1.box == (2, 63, 2, 23) and S2.box == (3, 62, 3, 22)
    L = S1.L
    plan3, other = C.c_void_p(), C.c_void_p()
    D._cabi.check(L.dlesm_halo_plan_create(C.byref(loopback_tables(D, D._cabi.Region(58, 18, 4, 61, 4, 21), 3)), 64, 24,
                                           C.byref(plan3)))
    D._cabi.check(L.dlesm_halo_plan_create(C.byref(S1.t), 66, 24, C.byref(other)))
    null = C.c_void_p(0)
    try:
        prm = D.psy.momentum_params(*PRM)
        (O1, c1), (O2, c2) = S1.outputs(), S2.outputs()
        by_depth = {1: (S1, O1, c1), 2: (S2, O2, c2)}
        uneq1 = (S1.box, S1.box, (2, 62, 2, 23))
        uneq2 = (S2.box, S2.box, (3, 61, 3, 22))
        box_text1 = (2, 63, 2, 23, 2, 63, 2, 23, 2, 62, 2, 23)
        box_text2 = (3, 62, 3, 22, 3, 62, 3, 22, 3, 61, 3, 22)
        cases = []          # (what, call, the whole text)

        for e in FLOW_ENTRIES:
            cases += [
                (e + ": a null plan", lambda e=e: _flow(S1, e, O1, prm, plan=null), NULL_PLAN % e),
                (e + ": a plan of other extents", lambda e=e: _flow(S1, e, O1, prm, plan=other), EXTENTS % e),
                (e + ": a depth-2 plan", lambda e=e: _flow(S2, e, O2, prm), DEPTH % (e, 2, 1, 1)),
                (e + ": unequal boxes", lambda e=e: _flow(S1, e, O1, prm, boxes=uneq1), ONE_BOX % ((e,) + box_text1)),
                # order
                (e + ": a depth-2 plan and unequal boxes", lambda e=e: _flow(S2, e, O2, prm, boxes=uneq2),
                 DEPTH % (e, 2, 1, 1)),
                (e + ": a null plan and unequal boxes", lambda e=e: _flow(S1, e, O1, prm, plan=null, boxes=uneq1),
                 NULL_PLAN % e),
            ]
        for e, d in TRACER_ENTRIES.items():
            S, O_, co = by_depth[d]                 # the plan the entry takes
            W, Ow, cw = by_depth[3 - d]             # the plan of the other depth
            nine_o, nine_i = [co[0]] * 9, [S.ci[0]] * 9
            cases += [
                (e + ": a null plan", lambda e=e, S=S, O_=O_, co=co: _tracers(S, e, O_, co, plan=null), NULL_PLAN % e),
                (e + ": a plan of other extents", lambda e=e, S=S, O_=O_, co=co: _tracers(S, e, O_, co, plan=other),
                 EXTENTS % e),
                (e + ": a depth-%d plan" % (3 - d), lambda e=e, W=W, Ow=Ow, cw=cw: _tracers(W, e, Ow, cw),
                 DEPTH % (e, 3 - d, d, d)),
                (e + ": 0 tracers", lambda e=e, S=S, O_=O_, co=co: _tracers(S, e, O_, co, k=0), "%s: 0 tracers (1..8)" % e),
                (e + ": 9 tracers", lambda e=e, S=S, O_=O_, a=nine_o, b=nine_i: _tracers(S, e, O_, a, ci=b),
                 "%s: 9 tracers (1..8)" % e),
                (e + ": c_out[0] twice", lambda e=e, S=S, O_=O_, co=co: _tracers(S, e, O_, [co[0], co[0]]),
                 "%s: c_out[0] and c_out[1] overlap" % e),
                (e + ": c_out[0] is c_in[1]", lambda e=e, S=S, O_=O_, co=co: _tracers(S, e, O_, [S.ci[1], co[1]]),
                 "%s: c_out[0] overlaps c_in[1]" % e),
                # order
                (e + ": a depth-%d plan and 9 tracers" % (3 - d),
                 lambda e=e, W=W, Ow=Ow, cw=cw: _tracers(W, e, Ow, [cw[0]] * 9, ci=[W.ci[0]] * 9), "%s: 9 tracers (1..8)" % e),
                (e + ": a null plan and 9 tracers", lambda e=e, S=S, O_=O_, a=nine_o, b=nine_i:
                 _tracers(S, e, O_, a, ci=b, plan=null), NULL_PLAN % e),
            ]
        e = COUPLED
        cases += [
            (e + ": a null plan", lambda: one_call(S2, "hancock", O2, c2, None, 0.0, prm, plan=null), NULL_PLAN % e),
            (e + ": a plan of other extents", lambda: one_call(S2, "hancock", O2, c2, None, 0.0, prm, plan=other), EXTENTS % e),
            (e + ": a depth-3 plan", lambda: one_call(S2, "upwind", O2, c2, None, 0.0, prm, plan=plan3), DEPTH_1_OR_2 % e),
            (e + ": a limited scheme with one tracer on a depth-1 plan",
             lambda: one_call(S1, "muscl", O1, c1[:1], None, 0.0, prm, k=1, ci=S1.ci[:1]), LIMITED % e),
            (e + ": scheme 3", lambda: one_call(S2, 3, O2, c2, None, 0.0, prm), "%s: scheme 3 (0 upwind, 1 MUSCL, 2 Hancock)" % e),
            (e + ": 9 tracers", lambda: one_call(S2, "upwind", O2, [c2[0]] * 9, None, 0.0, prm, k=9, ci=[S2.ci[0]] * 9),
             "%s: 9 tracers (0..8)" % e),
            (e + ": c_out[0] is ua", lambda: one_call(S2, "hancock", O2, [O2["ua"]], None, 0.0, prm, k=1, ci=S2.ci[:1]),
             "%s: c_out[0] overlaps ua" % e),
            (e + ": unequal boxes", lambda: one_call(S2, "hancock", O2, c2, None, 0.0, prm, boxes=uneq2),
             ONE_BOX % ((e,) + box_text2)),
            # order
            (e + ": a limited scheme on a depth-1 plan and unequal boxes",
             lambda: one_call(S1, "hancock", O1, c1[:1], None, 0.0, prm, k=1, ci=S1.ci[:1], boxes=uneq1), LIMITED % e),
            (e + ": scheme 3 and a plan of other extents", lambda: one_call(S2, 3, O2, c2, None, 0.0, prm, plan=other),
             EXTENTS % e),
            (e + ": a null plan and scheme 3", lambda: one_call(S2, 3, O2, c2, None, 0.0, prm, plan=null), NULL_PLAN % e),
        ]
        assert len(cases) == 2 * 6 + 3 * 9 + 11

        bad = []
        for what, call, text in cases:
            rc = call()
            err = L.dlesm_last_error()
            if rc != D._cabi.EINVAL or err != text.encode():
                bad.append((what, rc, err, text))
        assert not bad, bad

        torch.cuda.synchronize()
        for S, O_, co in ((S1, O1, c1), (S2, O2, c2)):
            for n in OUTS:
                assert M.same(O_[n].cpu().numpy(), S.Ho[n]), n
            for c in co:
                assert (c.cpu().numpy() == TC.SENTINEL).all()
            S.inputs_untouched()
    finally:
        L.dlesm_halo_plan_destroy(plan3)
        L.dlesm_halo_plan_destroy(other)
        S1.close()
        S2.close()
