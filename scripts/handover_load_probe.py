#!/usr/bin/env python3
"""One recorded measurement of the POWER of the hand-over tests (tests/test_a_handover_load_gpu.py), not a test: the
loop-back worker once per load pattern with the reader's acquire switched off (dm_acquire = 0) and once with relaxed
mailbox flags (mailbox_fences = 0) -- the two measurement-only forms of INTEGRATION.md, which change what a reader may see,
not whether a wait ends.  Records how many words differed per form.  Nothing is asserted: if no word differs, the tests
show that the valid forms hold under load, not that they would catch these invalid ones.

    python scripts/handover_load_probe.py [--out build/handover_load_probe.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="build/handover_load_probe.json")
    ap.add_argument("--patterns", default="none,few,lopsided,stream")
    args = ap.parse_args()
    import test_a_handover_load_gpu as T
    from handover_load import window_is_loaded
    res = []
    for key in ("dm_acquire", "mailbox_fences"):
        for pattern in args.patterns.split(","):
            outs, codes, load = T.run_under_load(pattern, 1, ["loopback", "--tune", f"{key}=0"])
            forms, total = {}, 0
            for ln in outs[0].splitlines():
                if ln.startswith("FORM "):
                    _, label, _, a, b, first = ln.split()
                    forms[label] = {"A": int(a[2:]), "B": int(b[2:]), "first_bad_step": int(first.split("=")[1])}
                    total += forms[label]["A"] + forms[label]["B"]
            wins = T.windows_of(outs[0])
            loaded = sum(1 for _, _, t0, t1 in wins if window_is_loaded(load["completions"], t0, t1))
            other = [ln for ln in outs[0].splitlines() if "ERROR" in ln and "pass " not in ln]
            res.append({"key": key, "value": 0, "pattern": pattern, "exit": codes[0], "forms_run": len(forms),
                        "words_differing": total, "forms_with_differences": {k: v for k, v in forms.items() if v["A"] or v["B"]},
                        "windows": len(wins), "windows_under_load": loaded, "load_launch_ms": load["launch_ms"],
                        "other_errors": other[:20]})
            print(f"{key}=0 under `{pattern}`: {len(forms)} forms, {total} words differ, {loaded} of {len(wins)} windows under load, "
                  f"exit {codes[0]}", flush=True)
            if codes[0] not in (0, 1):
                print("the worker died: stopping here", flush=True)
                break
        else:
            continue
        break
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
