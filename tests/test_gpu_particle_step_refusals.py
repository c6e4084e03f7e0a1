"""GPU test (-m gpu) that pins what the particle steps refuse, and in which order: dlesm_drifter_step_f64,
dlesm_dispersal_step_f64, dlesm_random_walk_f64, the two _set forms and dlesm_drifter_sample_f64.  Every single fault keeps its
return code and its WHOLE text; for pairs of faults the one that is reported is pinned -- a shared rule against the entry's own
rule, the entry's own rule against a rule of the random stream, a rule of the stream against an overlap with kh_t, the set
guard against everything behind it.  The shapes are those of the three files' refusal tests: n = 257, ld = 26, DC.NY,
DC.BOXES[0].  Nothing is launched: after all the calls every array holds what it held.  The texts are literals written from
the format strings."""
import ctypes as C

import numpy as np
import pytest

import drifter_cases as DC
import random_walk_cases as RC
from particle_gpu import SENT, SLACK, T, _flow, _particles, _up  # noqa: F401  (T is the fixture)

pytestmark = pytest.mark.gpu

N, LD, NY, BOX = 257, 26, DC.NY, DC.BOXES[0]
STEP, DISP, WALK = "dlesm_drifter_step_f64", "dlesm_dispersal_step_f64", "dlesm_random_walk_f64"
DISP_SET, WALK_SET, SAMPLE = "dlesm_dispersal_step_set", "dlesm_random_walk_set", "dlesm_drifter_sample_f64"
IN_NAME = ["tmask", "dx_t", "dy_t", "un", "vn"]
P_NAME = ["px", "py", "status"]
RING = "%s: box (%d:%d,%d:%d) with a 1-cell stencil ring does not fit in an array of 26x22"


def _vp(p):
    return C.c_void_p(p) if p else None


def test_every_refusal_keeps_its_code_its_place_and_its_text(T):
    torch, D, L = T
    assert NY == 22
    MAX_SUB, MAX_FIELDS = D._cabi.DRIFTER_MAX_SUB, D._cabi.DRIFTER_MAX_FIELDS
    F = _flow(torch, LD, 0)
    K = _up(torch, RC.kh_field())
    P = _particles(torch, N)
    ids = _up(torch, RC.ids()[:N + SLACK].copy())
    tk = torch.full((2,), 11, dtype=torch.int64, device="cuda")
    host = DC.sample_fields(2)
    Sf = [_up(torch, f) for f in host]
    So = [_up(torch, np.full(N, SENT)) for _ in host]
    kept = P + [ids, tk, K] + F + Sf + So
    before = [t.clone() for t in kept]
    Fp, Pp = [t.data_ptr() for t in F], [t.data_ptr() for t in P]
    fp, op = [t.data_ptr() for t in Sf], [t.data_ptr() for t in So]
    kh_last = K.data_ptr() + 8 * (LD * NY) - 8
    # two allocations of their own, so that what lies beside an array decides nothing: ids whose last element is the first of a
    # status array behind them, and a kh_t whose last element is the first of a particle array behind it
    room = torch.full((2 * N,), -9, dtype=torch.int32, device="cuda")
    wide = torch.full((LD * NY + N,), SENT, dtype=torch.float64, device="cuda")
    wide_last = wide.data_ptr() + 8 * (LD * NY) - 8
    kept, before = kept + [room, wide], before + [room.clone(), wide.clone()]

    def step(e, Fq=Fp, Pq=Pp, n=N, nsub=1, h=DC.H, b=BOX, ny=NY, ld=LD, kh=None, tick=0, id_=ids.data_ptr(),
             td=tk.data_ptr(), set_=None):
        """entry e with one or two arguments swapped; kh: dispersal's number or the walk's address (0: a null pointer)"""
        tail = [ld, ny, *b, *[_vp(p) for p in Fq]]
        if e == STEP:
            return L.dlesm_drifter_step_f64(h, nsub, *tail, n, *[_vp(p) for p in Pq], None)
        walk = e in (WALK, WALK_SET)
        kh = (_vp(K.data_ptr() if kh is None else kh)) if walk else (37.5 if kh is None else kh)
        head = [h, nsub, kh, 7, tick, _vp(td)]
        if e in (DISP_SET, WALK_SET):
            return getattr(L, e)(set_, *head, *tail, None)
        return getattr(L, e)(*head, *tail, n, _vp(id_), *[_vp(p) for p in Pq], None)

    def sample(fields=fp, outs=op, nf=2, n=N, parts=Pp, b=BOX, ld=LD, ny=NY):
        pf = (C.c_void_p * max(len(fields), 1))(*fields) if fields is not None else None
        po = (C.c_void_p * max(len(outs), 1))(*outs) if outs is not None else None
        return L.dlesm_drifter_sample_f64(ld, ny, *b, n, *[_vp(p) for p in parts], pf, po, nf, None)

    def swapped(a, k, value):
        q = list(a)
        q[k] = value
        return q

    cases = []          # (what, call, the whole text)

    def case(what, fn, text):
        cases.append((what, fn, text))

    # ---- the rules every step shares, under each entry's own name, in the order they are looked at
    for e in (STEP, DISP, WALK):
        for h, txt in ((float("nan"), "nan"), (float("inf"), "inf"), (float("-inf"), "-inf")):
            case(e + ": h = " + txt, lambda e=e, h=h: step(e, h=h), "%s: h = %s (a finite number of seconds)" % (e, txt))
        for nsub in (0, MAX_SUB + 1):
            case(e + ": nsub = %d" % nsub, lambda e=e, s=nsub: step(e, nsub=s), "%s: nsub = %d (1..%d)" % (e, nsub, MAX_SUB))
        case(e + ": a null mask", lambda e=e: step(e, Fq=swapped(Fp, 0, 0)), "%s: null tmask" % e)
        case(e + ": the mask two bytes on", lambda e=e: step(e, Fq=swapped(Fp, 0, Fp[0] + 2)), "%s: tmask is not 4-byte aligned" % e)
        for k in range(1, 5):
            case(e + ": a null " + IN_NAME[k], lambda e=e, k=k: step(e, Fq=swapped(Fp, k, 0)), "%s: null %s" % (e, IN_NAME[k]))
            case(e + ": %s four bytes on" % IN_NAME[k], lambda e=e, k=k: step(e, Fq=swapped(Fp, k, Fp[k] + 4)),
                 "%s: %s is not 8-byte aligned" % (e, IN_NAME[k]))
        for k in range(3):
            case(e + ": a null " + P_NAME[k], lambda e=e, k=k: step(e, Pq=swapped(Pp, k, 0)), "%s: null px, py or status" % e)
        for k in range(2):
            case(e + ": %s four bytes on" % P_NAME[k], lambda e=e, k=k: step(e, Pq=swapped(Pp, k, Pp[k] + 4)),
                 "%s: px or py is not 8-byte aligned" % e)
        case(e + ": status two bytes on", lambda e=e: step(e, Pq=swapped(Pp, 2, Pp[2] + 2)), "%s: status is not 4-byte aligned" % e)
        case(e + ": n = -1", lambda e=e: step(e, n=-1), "%s: -1 particles" % e)
        case(e + ": ld = 0", lambda e=e: step(e, ld=0), "%s: array extents 0x22" % e)
        case(e + ": ny = 0", lambda e=e: step(e, ny=0), "%s: array extents 26x0" % e)
        for b in ((1, 25, 2, 21), (2, 26, 2, 21), (2, 25, 1, 21), (2, 25, 2, 22)):
            case(e + ": no room for the ring %r" % (b,), lambda e=e, b=b: step(e, b=b), RING % ((e,) + b))
        case(e + ": px in the mask", lambda e=e: step(e, Pq=swapped(Pp, 0, Fp[0])), "%s: px overlaps tmask" % e)
        case(e + ": status on the mask's last element", lambda e=e: step(e, Pq=swapped(Pp, 2, Fp[0] + 4 * (LD * NY) - 4), n=1),
             "%s: status overlaps tmask" % e)
        for k in range(1, 5):
            case(e + ": px in " + IN_NAME[k], lambda e=e, k=k: step(e, Pq=swapped(Pp, 0, Fp[k])),
                 "%s: px overlaps the input %s" % (e, IN_NAME[k]))
            case(e + ": status in " + IN_NAME[k], lambda e=e, k=k: step(e, Pq=swapped(Pp, 2, Fp[k])),
                 "%s: status overlaps the input %s" % (e, IN_NAME[k]))
        case(e + ": py is px", lambda e=e: step(e, Pq=swapped(Pp, 1, Pp[0])), "%s: px and py overlap" % e)
        case(e + ": py on px's last element", lambda e=e: step(e, Pq=swapped(Pp, 1, Pp[0] + 8 * (N - 1))), "%s: px and py overlap" % e)
        case(e + ": status is px", lambda e=e: step(e, Pq=swapped(Pp, 2, Pp[0])), "%s: px and status overlap" % e)
        case(e + ": status is py", lambda e=e: step(e, Pq=swapped(Pp, 2, Pp[1])), "%s: py and status overlap" % e)
        # order inside the shared rules
        case(e + ": h and nsub", lambda e=e: step(e, h=float("nan"), nsub=0), "%s: h = nan (a finite number of seconds)" % e)
        case(e + ": nsub and a null un", lambda e=e: step(e, nsub=0, Fq=swapped(Fp, 3, 0)), "%s: nsub = 0 (1..%d)" % (e, MAX_SUB))
        case(e + ": a null un and n = -1", lambda e=e: step(e, Fq=swapped(Fp, 3, 0), n=-1), "%s: null un" % e)
        case(e + ": n = -1 and no room for the ring", lambda e=e: step(e, n=-1, b=(1, 25, 2, 21)), "%s: -1 particles" % e)
        case(e + ": no room for the ring and py is px", lambda e=e: step(e, b=(1, 25, 2, 21), Pq=swapped(Pp, 1, Pp[0])),
             RING % (e, 1, 25, 2, 21))

    # ---- the rules of the random stream, for the two entries that draw numbers
    for e in (DISP, WALK):
        TICK = "%s: tick = %d (>= 0, tick + nsub representable)"
        case(e + ": tick = -1", lambda e=e: step(e, tick=-1), TICK % (e, -1))
        case(e + ": tick = 2^63 - 1", lambda e=e: step(e, tick=2 ** 63 - 1), TICK % (e, 2 ** 63 - 1))
        case(e + ": tick + nsub = 2^63", lambda e=e: step(e, tick=2 ** 63 - 3, nsub=3), TICK % (e, 2 ** 63 - 3))
        case(e + ": id two bytes on", lambda e=e: step(e, id_=ids.data_ptr() + 2), "%s: id is not 4-byte aligned" % e)
        case(e + ": tick_dev four bytes on", lambda e=e: step(e, td=tk.data_ptr() + 4), "%s: tick_dev is not 8-byte aligned" % e)
        for k in range(3):
            case(e + ": id is " + P_NAME[k], lambda e=e, k=k: step(e, id_=Pp[k]), "%s: id overlaps %s" % (e, P_NAME[k]))
            case(e + ": tick_dev in " + P_NAME[k], lambda e=e, k=k: step(e, td=Pp[k] + 8), "%s: tick_dev overlaps %s" % (e, P_NAME[k]))
        case(e + ": the last id is the first status",
             lambda e=e: step(e, id_=room.data_ptr() + 4, Pq=swapped(Pp, 2, room.data_ptr() + 4 * N)), "%s: id overlaps status" % e)
        for k in range(5):
            case(e + ": tick_dev in " + IN_NAME[k], lambda e=e, k=k: step(e, td=Fp[k] + 8),
                 "%s: tick_dev overlaps the input %s" % (e, IN_NAME[k]))
        case(e + ": tick_dev on the mask's last eight bytes", lambda e=e: step(e, td=Fp[0] + 4 * (LD * NY) - 8),
             "%s: tick_dev overlaps the input tmask" % e)
        case(e + ": tick_dev in id", lambda e=e: step(e, td=ids.data_ptr() + 8), "%s: tick_dev overlaps the input id" % e)
        # order inside the stream's rules
        case(e + ": tick and id", lambda e=e: step(e, tick=-1, id_=ids.data_ptr() + 2), TICK % (e, -1))
        case(e + ": id is px and tick_dev in an input", lambda e=e: step(e, id_=Pp[0], td=Fp[1] + 8), "%s: id overlaps px" % e)
        # a seam: a shared rule -- the last of them -- is found before a rule of the stream
        case(e + ": status is py and tick", lambda e=e: step(e, Pq=swapped(Pp, 2, Pp[1]), tick=-1), "%s: py and status overlap" % e)

    # ---- dlesm_dispersal_step_f64's own rule, between the shared rules and the stream's
    KH = DISP + ": kh = %s (a finite diffusivity >= 0 in m2/s)"
    for kh, txt in ((-1.0, "-1"), (-5e-324, "-4.94066e-324"), (float("nan"), "nan"), (float("inf"), "inf"), (float("-inf"), "-inf")):
        case(DISP + ": kh = " + txt, lambda kh=kh: step(DISP, kh=kh), KH % txt)
    case(DISP + ": nsub and kh", lambda: step(DISP, nsub=0, kh=-1.0), "%s: nsub = 0 (1..%d)" % (DISP, MAX_SUB))
    case(DISP + ": status is py and kh", lambda: step(DISP, Pq=swapped(Pp, 2, Pp[1]), kh=-1.0), DISP + ": py and status overlap")
    case(DISP + ": kh and tick", lambda: step(DISP, kh=-1.0, tick=-1), KH % "-1")
    case(DISP + ": kh and tick_dev in id", lambda: step(DISP, kh=-1.0, td=ids.data_ptr() + 8), KH % "-1")

    # ---- dlesm_random_walk_f64's own rules, behind the stream's
    case(WALK + ": a null kh_t", lambda: step(WALK, kh=0), WALK + ": null kh_t")
    case(WALK + ": kh_t four bytes on", lambda: step(WALK, kh=K.data_ptr() + 4), WALK + ": kh_t is not 8-byte aligned")
    for k in range(3):
        case(WALK + ": %s on kh_t's last element" % P_NAME[k], lambda k=k: step(WALK, Pq=swapped(Pp, k, kh_last), n=1),
             "%s: %s overlaps the input kh_t" % (WALK, P_NAME[k]))
        case(WALK + ": kh_t's last element is %s's first" % P_NAME[k], lambda k=k: step(WALK, kh=wide.data_ptr(), Pq=swapped(Pp, k, wide_last)),
             "%s: %s overlaps the input kh_t" % (WALK, P_NAME[k]))
    case(WALK + ": tick_dev is kh_t's first element", lambda: step(WALK, td=K.data_ptr()), WALK + ": tick_dev overlaps the input kh_t")
    case(WALK + ": tick_dev is kh_t's last element", lambda: step(WALK, td=kh_last), WALK + ": tick_dev overlaps the input kh_t")
    case(WALK + ": nsub and a null kh_t", lambda: step(WALK, nsub=0, kh=0), "%s: nsub = 0 (1..%d)" % (WALK, MAX_SUB))
    case(WALK + ": tick and a null kh_t", lambda: step(WALK, tick=-1, kh=0), "%s: tick = -1 (>= 0, tick + nsub representable)" % WALK)
    case(WALK + ": tick_dev in id and a null kh_t", lambda: step(WALK, td=ids.data_ptr() + 8, kh=0),
         WALK + ": tick_dev overlaps the input id")
    case(WALK + ": id two bytes on and px in kh_t", lambda: step(WALK, id_=ids.data_ptr() + 2, Pq=swapped(Pp, 0, kh_last), n=1),
         WALK + ": id is not 4-byte aligned")
    case(WALK + ": kh_t is vn and tick_dev in both", lambda: step(WALK, kh=Fp[4], td=Fp[4] + 8),
         WALK + ": tick_dev overlaps the input vn")
    case(WALK + ": kh_t four bytes on and px in kh_t",
         lambda: step(WALK, kh=K.data_ptr() + 4, Pq=swapped(Pp, 0, kh_last), n=1), WALK + ": kh_t is not 8-byte aligned")
    case(WALK + ": px in kh_t and tick_dev in kh_t", lambda: step(WALK, Pq=swapped(Pp, 0, kh_last), n=1, td=K.data_ptr()),
         WALK + ": px overlaps the input kh_t")

    # ---- the two _set forms: the guard first, then the array form's refusals under the array form's name
    rc = C.c_void_p()
    assert L.dlesm_drifters_create(N, C.byref(rc)) == 0 and rc.value
    full = rc
    rc = C.c_void_p()
    assert L.dlesm_drifters_create(0, C.byref(rc)) == 0 and rc.value
    none = rc
    junk = C.create_string_buffer(256)                                              # no magic in it
    for e, f64 in ((DISP_SET, DISP), (WALK_SET, WALK)):
        for what, s in (("a null set", None), ("something that is no set", C.cast(junk, C.c_void_p))):
            case(e + ": " + what, lambda e=e, s=s: step(e, set_=s), "%s: not a drifter set" % e)
            case(e + ": %s and nsub" % what, lambda e=e, s=s: step(e, set_=s, nsub=0), "%s: not a drifter set" % e)
        case(e + ": nsub", lambda e=e: step(e, set_=full, nsub=0), "%s: nsub = 0 (1..%d)" % (f64, MAX_SUB))
        case(e + ": tick", lambda e=e: step(e, set_=full, tick=-1), "%s: tick = -1 (>= 0, tick + nsub representable)" % f64)
        case(e + ": a null un", lambda e=e: step(e, set_=full, Fq=swapped(Fp, 3, 0)), "%s: null un" % f64)
        case(e + ": no room for the ring", lambda e=e: step(e, set_=full, b=(2, 26, 2, 21)), RING % (f64, 2, 26, 2, 21))
    case(DISP_SET + ": kh", lambda: step(DISP_SET, set_=full, kh=-1.0), KH % "-1")
    case(WALK_SET + ": a null kh_t", lambda: step(WALK_SET, set_=full, kh=0), WALK + ": null kh_t")

    # ---- dlesm_drifter_sample_f64: its own rules, then the particle rules it shares with the steps, then its overlaps
    e = SAMPLE
    NF = e + ": nfields = %d (1..%d)"
    case(e + ": no field", lambda: sample(nf=0), NF % (0, MAX_FIELDS))
    case(e + ": nine fields", lambda: sample(fp * 5, op * 5, 9), NF % (9, MAX_FIELDS))
    case(e + ": null fields", lambda: sample(fields=None), e + ": null fields or out")
    case(e + ": null out", lambda: sample(outs=None), e + ": null fields or out")
    case(e + ": a null fields[1]", lambda: sample(fields=[fp[0], None]), e + ": null fields[1] or out[1]")
    case(e + ": a null out[0]", lambda: sample(outs=[None, op[1]]), e + ": null fields[0] or out[0]")
    case(e + ": fields[1] four bytes on", lambda: sample(fields=[fp[0], fp[1] + 4]), e + ": fields[1] or out[1] is not 8-byte aligned")
    case(e + ": out[0] four bytes on", lambda: sample(outs=[op[0] + 4, op[1]]), e + ": fields[0] or out[0] is not 8-byte aligned")
    for k in range(3):
        case(e + ": a null " + P_NAME[k], lambda k=k: sample(parts=swapped(Pp, k, 0)), e + ": null px, py or status")
    case(e + ": py four bytes on", lambda: sample(parts=swapped(Pp, 1, Pp[1] + 4)), e + ": px or py is not 8-byte aligned")
    case(e + ": status two bytes on", lambda: sample(parts=swapped(Pp, 2, Pp[2] + 2)), e + ": status is not 4-byte aligned")
    case(e + ": n = -1", lambda: sample(n=-1), e + ": -1 particles")
    case(e + ": ld = 0", lambda: sample(ld=0), e + ": array extents 0x22")
    case(e + ": no room for the ring", lambda: sample(b=(1, 25, 2, 21)), RING % (e, 1, 25, 2, 21))
    for k in range(3):
        case(e + ": out[1] is " + P_NAME[k], lambda k=k: sample(outs=[op[0], Pp[k]]), "%s: out[1] overlaps %s" % (e, P_NAME[k]))
    case(e + ": out[1] is fields[0]", lambda: sample(outs=[op[0], fp[0]]), e + ": out[1] overlaps fields[0]")
    case(e + ": out[0] is on fields[1]'s last element", lambda: sample(outs=[fp[1] + 8 * (LD * NY) - 8, op[1]], n=1),
         e + ": out[0] overlaps fields[1]")
    case(e + ": out[1] is out[0]", lambda: sample(outs=[op[0], op[0]]), e + ": out[0] and out[1] overlap")
    # order
    case(e + ": no field and n = -1", lambda: sample(nf=0, n=-1), NF % (0, MAX_FIELDS))
    case(e + ": a null out[0] and a null px", lambda: sample(outs=[None, op[1]], parts=swapped(Pp, 0, 0)),
         e + ": null fields[0] or out[0]")
    case(e + ": a null px and out[1] is out[0]", lambda: sample(parts=swapped(Pp, 0, 0), outs=[op[0], op[0]]),
         e + ": null px, py or status")
    case(e + ": n = -1 and no room for the ring", lambda: sample(n=-1, b=(1, 25, 2, 21)), e + ": -1 particles")
    case(e + ": out[0] is px and out[1] is out[0]", lambda: sample(outs=[Pp[0], Pp[0]]), e + ": out[0] overlaps px")

    #                  shared + order   stream + order + seam   kh    walk   sets         sample
    assert len(cases) == 3 * (42 + 5) + 2 * (19 + 2 + 1) + 9 + 17 + (2 * 8 + 2) + (22 + 5)

    try:
        bad = []
        for what, fn, text in cases:
            rc = fn()
            err = L.dlesm_last_error()
            if rc != D._cabi.EINVAL or err != text.encode():
                bad.append((what, rc, err, text))
        assert not bad, bad

        # what is no fault: no particles, an empty box, an empty set whatever else is asked of it
        for e in (STEP, DISP, WALK):
            assert step(e, n=0) == 0 and step(e, b=(5, 4, 2, 21)) == 0 and step(e, b=(2, 25, 9, 8)) == 0, e
        assert step(DISP_SET, set_=none, nsub=0) == 0 and step(WALK_SET, set_=none, kh=0) == 0
        assert sample(n=0) == 0 and sample(b=(5, 4, 2, 21)) == 0

        torch.cuda.synchronize()
        for a, b_ in zip(kept, before):
            assert torch.equal(a.view(torch.int32), b_.view(torch.int32))
        gs = np.full(N, -1, dtype=np.int32)
        assert L.dlesm_drifters_get(full, None, None, gs.ctypes.data) == 0 and (gs == 0).all()
    finally:
        assert L.dlesm_drifters_destroy(full) == 0 and L.dlesm_drifters_destroy(none) == 0
