"""GPU test (-m gpu) that pins what the 17 shallow-water entries refuse, and in which order: the single-domain steps
(dlesm_shallow_step_f64, _sw_f64, _sw_periodic_f64, _smooth_f64, _sw_smooth_periodic_f64), the two planning calls, the four
two-step entries and the six distributed ones.  Every refusal keeps its return code, its place among the refusals and its
WHOLE text.  One process, loop-back on one GPU: 64 x 24 arrays with the box (2:63, 2:23) on a depth-1 plan and the box
(3:62, 3:22) on a depth-2 plan, and a plan made for 66 x 24 arrays.  Nothing is launched: after all the calls every output
still holds its sentinel and every input its values.  The texts are literals written from the format strings.

What does not apply: the four one-step distributed entries do not look at the nine pointers themselves (the single-domain step
they fall back to does), so they have no null-field and no alias case; their box is checked under the name
dlesm_shallow_step_dm by the one-launch form."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

LD, NY = 64, 24
BOX1, BOX2 = (2, 63, 2, 23), (3, 62, 3, 22)
SENTINEL = 9.0

NULLP = "null pointer"
BOX = "%s: box (%d:%d,%d:%d) with a %d-cell stencil ring does not fit in an array of 64x24"
ALIAS = "shallow step: outputs alias the 3x3-read inputs"
ALIAS_EACH = "shallow step: outputs alias the 3x3-read inputs or each other"
NINE = "%s: the nine fields must be nine different arrays"
OVERLAP = "%s: the twelve arrays must not overlap (arguments %d and %d do)"
EXTENTS = "plan is for 66x24 fields, got 64x24"
DEPTH = "%s: the plan exchanges depth-1 halos, two steps per launch need depth 2 (dlesm_map_comms_depth, depth = 2)"

# entry -> (plan argument?, alpha argument?, region + bc_x, bc_y instead of the four box integers?, arrays)
ENTRIES = {
    "dlesm_shallow_step_f64": (0, 0, 0, 9),
    "dlesm_shallow_step_sw_f64": (0, 0, 0, 9),
    "dlesm_shallow_autotune_f64": (0, 0, 0, 9),
    "dlesm_shallow_autotune_sw_f64": (0, 0, 0, 9),
    "dlesm_shallow_step_sw_periodic_f64": (0, 0, 1, 9),
    "dlesm_shallow_step_smooth_f64": (0, 1, 0, 9),
    "dlesm_shallow_step_sw_smooth_periodic_f64": (0, 1, 1, 9),
    "dlesm_shallow_step_x2_f64": (0, 0, 0, 12),
    "dlesm_shallow_step_smooth_x2_f64": (0, 1, 0, 12),
    "dlesm_shallow_step_sw_x2_periodic_f64": (0, 0, 1, 12),
    "dlesm_shallow_step_sw_smooth_x2_periodic_f64": (0, 1, 1, 12),
    "dlesm_shallow_step_dm": (1, 0, 0, 9),
    "dlesm_shallow_step_dm_pipelined": (1, 0, 0, 9),
    "dlesm_shallow_step_smooth_dm": (1, 1, 0, 9),
    "dlesm_shallow_step_smooth_dm_pipelined": (1, 1, 0, 9),
    "dlesm_shallow_step_x2_dm": (1, 0, 0, 12),
    "dlesm_shallow_step_smooth_x2_dm": (1, 1, 0, 12),
}
# the name in front of the box text: the planning calls run the step first; the one-step distributed entries share one check
BOX_NAME = {"dlesm_shallow_autotune_f64": "dlesm_shallow_step_f64", "dlesm_shallow_autotune_sw_f64": "dlesm_shallow_step_sw_f64",
            "dlesm_shallow_step_dm_pipelined": "dlesm_shallow_step_dm", "dlesm_shallow_step_smooth_dm": "dlesm_shallow_step_dm",
            "dlesm_shallow_step_smooth_dm_pipelined": "dlesm_shallow_step_dm"}


@pytest.fixture(scope="module")
def D():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU")
    import dl_esm_inf_amd as d
    torch.cuda.set_device(0)
    d.parallel_init(0, 1, use_rccl=True)
    return d


def test_every_refusal_keeps_its_code_its_place_and_its_text(D):
    import torch
    from dm_overhead import loopback_tables
    L = D._cabi.lib()
    Region = D._cabi.Region
    prm = D.psy.shallow_params(1.0e5, 1.0e5, 90.0)
    rng = np.random.default_rng(64 * 24)
    Hin = [rng.random((NY, LD)) + (1.0 if k % 3 == 2 else -0.5) for k in range(6)]
    ins = [torch.from_numpy(h).cuda() for h in Hin]
    outs = [torch.full((NY, LD), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(6)]
    tall = torch.full((NY + 2, LD), SENTINEL, dtype=torch.float64, device="cuda")   # an array and its alias two rows further
    good = [t.data_ptr() for t in ins + outs]
    shifted = tall.data_ptr() + 2 * LD * 8

    t1 = loopback_tables(D, Region(62, 22, *BOX1), 1)
    t2 = loopback_tables(D, Region(60, 20, *BOX2), 2)
    plan1, plan2, other = C.c_void_p(), C.c_void_p(), C.c_void_p()
    D._cabi.check(L.dlesm_halo_plan_create(C.byref(t1), LD, NY, C.byref(plan1)))
    D._cabi.check(L.dlesm_halo_plan_create(C.byref(t2), LD, NY, C.byref(plan2)))
    D._cabi.check(L.dlesm_halo_plan_create(C.byref(t1), 66, NY, C.byref(other)))
    null = C.c_void_p(0)

    def call(e, box=None, ptrs=None, q=True, plan=None, region=True):
        has_plan, has_alpha, by_region, n = ENTRIES[e]
        two = n == 12
        box = box or (BOX2 if has_plan and two else BOX1)
        a = []
        if has_plan:
            a.append((plan2 if two else plan1) if plan is None else plan)
        a.append(C.byref(prm) if q else None)
        if has_alpha:
            a.append(0.001)
        a += [LD, NY]
        if by_region:
            a += [C.byref(Region(box[1] - box[0] + 1, box[3] - box[2] + 1, *box)) if region else None, D.GO_BC_PERIODIC,
                  D.GO_BC_PERIODIC]
        else:
            a += list(box)
        a += [C.c_void_p(x) if x else None for x in (ptrs or good)[:n]]
        return getattr(L, e)(*a, None)

    def swapped(k, value):
        p = list(good)
        p[k] = value
        return p

    cases = []          # (what, call, the whole text)
    for e, (has_plan, has_alpha, by_region, n) in ENTRIES.items():
        bname = BOX_NAME.get(e, e)
        outside = (2, 63, 2, 23) if has_plan and n == 12 else (1, 64, 2, 23)
        ring = 2 if has_plan and n == 12 else 1
        box_text = BOX % ((bname,) + outside + (ring,))
        cases += [(e + ": a null q", lambda e=e: call(e, q=False), NULLP),
                  (e + ": a box outside the array", lambda e=e, b=outside: call(e, box=b), box_text)]
        if by_region:
            cases += [(e + ": a null region", lambda e=e: call(e, region=False), NULLP)]
        if has_plan:
            cases += [(e + ": a null plan", lambda e=e: call(e, plan=null), NULLP),
                      (e + ": a plan of other extents", lambda e=e: call(e, plan=other), EXTENTS),
                      # order
                      (e + ": a null q and a plan of other extents", lambda e=e: call(e, q=False, plan=other), NULLP),
                      (e + ": a plan of other extents and a box outside the array",
                       lambda e=e, b=outside: call(e, plan=other, box=b), EXTENTS)]
        if has_plan and n == 9:
            continue                                     # (the nine pointers are the single-domain step's to check)
        for k in (0, 4, n - 1):
            cases += [(e + ": a null field %d" % k, lambda e=e, k=k: call(e, ptrs=swapped(k, 0)), NULLP)]
        # order: the null field is found before the box is looked at
        cases += [(e + ": a null field and a box outside the array",
                   lambda e=e, b=outside: call(e, box=b, ptrs=swapped(7, 0)), NULLP)]
        if n == 12:
            equal, two_rows = swapped(6, good[0]), swapped(9, shifted)
            two_rows[0] = tall.data_ptr()
            # (the text counts in the order of the kernel's array list, in which dlesm_shallow_step_smooth_x2_dm puts the
            # filtered level n+1 -- its arguments 9..11 -- before level n+2)
            at6, at9 = (9, 6) if e == "dlesm_shallow_step_smooth_x2_dm" else (6, 9)
            cases += [(e + ": argument 6 is argument 0", lambda e=e, p=equal: call(e, ptrs=p), OVERLAP % (e, 0, at6)),
                      (e + ": argument 9 is argument 0 two rows further", lambda e=e, p=two_rows: call(e, ptrs=p),
                       OVERLAP % (e, 0, at9))]
            if has_plan:
                cases += [(e + ": a depth-1 plan", lambda e=e: call(e, plan=plan1), DEPTH % e),
                          # order
                          (e + ": an overlap and a depth-1 plan", lambda e=e, p=equal: call(e, plan=plan1, ptrs=p),
                           OVERLAP % (e, 0, at6)),
                          (e + ": a depth-1 plan and a box outside the array",
                           lambda e=e, b=outside: call(e, plan=plan1, box=b), DEPTH % e),
                          (e + ": a plan of other extents and an overlap", lambda e=e, p=equal: call(e, plan=other, ptrs=p),
                           EXTENTS)]
            else:
                cases += [(e + ": a box outside the array and an overlap",
                           lambda e=e, b=outside, p=equal: call(e, box=b, ptrs=p), box_text)]
            continue
        if has_alpha:
            alias = [(e + ": uold is unew", swapped(3, good[6]), NINE % e), (e + ": u is v", swapped(1, good[0]), NINE % e)]
        elif e == "dlesm_shallow_step_sw_periodic_f64":
            alias = [(e + ": unew is u", swapped(6, good[0]), ALIAS_EACH), (e + ": unew is vnew", swapped(7, good[6]), ALIAS_EACH)]
        else:
            alias = [(e + ": unew is u", swapped(6, good[0]), ALIAS), (e + ": pnew is v", swapped(8, good[1]), ALIAS)]
        cases += [(what, lambda e=e, p=p: call(e, ptrs=p), text) for what, p, text in alias]
        # order: the box is looked at before the aliases
        cases += [(e + ": a box outside the array and an alias", lambda e=e, b=outside, p=alias[0][1]: call(e, box=b, ptrs=p),
                   box_text)]
    #          q, box   region  plan: 4   null fields + order: 4   overlaps / aliases and their order cases
    assert len(cases) == 17 * 2 + 4 + 6 * 4 + 13 * 4 + (4 * 3 + 2 * 6) + 7 * 3

    try:
        bad = []
        for what, fn, text in cases:
            rc = fn()
            err = L.dlesm_last_error()
            if rc != D._cabi.EINVAL or err != text.encode():
                bad.append((what, rc, err, text))
        assert not bad, bad

        torch.cuda.synchronize()
        for k in range(6):
            assert np.array_equal(ins[k].cpu().numpy(), Hin[k]), ("input", k)
            assert (outs[k].cpu().numpy() == SENTINEL).all(), ("output", k)
        assert (tall.cpu().numpy() == SENTINEL).all()
    finally:
        for p in (plan1, plan2, other):
            L.dlesm_halo_plan_destroy(p)
