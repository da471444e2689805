#!/usr/bin/env python3
"""Digests of gsv.serving.plan_online traces over the seeded cases of tests/_serving_cases.py (CPU only, no GPU, no torch).

For every seed of TRACE_SEEDS and every variant of TRACE_VARIANTS (plain, with `exclusive`, with `cfm_folds`, with `streaming`,
with both) the sha256 of repr(plan_online(..., with_steps=True)).  tests/serving_traces.json holds the digests of the commit
named in it, the last one before Scheduler and plan_online shared one step driver; tests/test_serving_traces.py recomputes them.
That file pins the schedule: it is written once, with --write on the commit whose schedule is the reference, and is not
regenerated to follow a change of serving.py -- a change of schedule that is meant gets a new file in a pull request of its own.

    tools/record_serving_traces.py                  compare against tests/serving_traces.json, exit 1 on a mismatch
    tools/record_serving_traces.py --write COMMIT   write tests/serving_traces.json, naming COMMIT as the reference
    tools/record_serving_traces.py --time N         best of N wall times of plan_online over all the cases
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gpt-sovits_amd"), os.path.join(ROOT, "tests")]
PATH = os.path.join(ROOT, "tests", "serving_traces.json")


def digests():
    from _serving_cases import TRACE_SEEDS, TRACE_VARIANTS, trace_case
    from gsv.serving import plan_online
    return {v: [hashlib.sha256(repr(plan_online(**trace_case(s, v), with_steps=True)).encode()).hexdigest() for s in TRACE_SEEDS]
            for v in TRACE_VARIANTS}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", metavar="COMMIT")
    ap.add_argument("--time", type=int, metavar="N")
    a = ap.parse_args()
    if a.time:
        best = min(_timed() for _ in range(a.time))
        print(json.dumps({"record": "plan_online_cpu", "cases": 1000, "best_of": a.time, "seconds": round(best, 4)}))
        return 0
    got = digests()
    if a.write:
        with open(PATH, "w") as f:
            json.dump({"commit": a.write, "digests": got}, f, indent=0, sort_keys=True)
            f.write("\n")
        return 0
    with open(PATH) as f:
        want = json.load(f)["digests"]
    bad = [(v, s) for v in want for s, (x, y) in enumerate(zip(want[v], got.get(v, []))) if x != y]
    print(f"{sum(len(d) for d in want.values())} traces, {len(bad)} differ" + (f": {bad[:10]}" if bad else ""))
    return 1 if bad or sorted(want) != sorted(got) else 0


def _timed():
    t0 = time.perf_counter()
    digests()
    return time.perf_counter() - t0


if __name__ == "__main__":
    sys.exit(main())
