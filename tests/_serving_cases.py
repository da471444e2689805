"""The seeded random cases of the gsv.serving.plan_online tests, shared by test_serving_plan.py, test_serving_cfm_plan.py,
test_serving_stream_plan.py and the recorded traces (tools/record_serving_traces.py, test_serving_traces.py).  A change here
changes the recorded cases: the generators draw from `random.Random(seed)` in a fixed order."""
import random


def plan_case(seed, closed=False, with_exclusive=True):
    """slots 1-8, chunk 1-16, arrivals spread over 0-20 steps (closed: all at step 0, no exclusive request)"""
    rng = random.Random(seed)
    n = rng.randint(1, 9)
    slots, chunk = rng.randint(1, 8), rng.randint(1, 16)
    admit_min = rng.choice([None, 1, rng.randint(1, slots)])
    wave_hold = rng.choice([0, 0, 1, 3])
    arrivals = [0] * n if closed else sorted(rng.randint(0, 20) for _ in range(n))
    if not closed and rng.random() < 0.5:
        rng.shuffle(arrivals)                       # request numbers need not follow arrival order
    exclusive = {r for r in range(n) if with_exclusive and not closed and rng.random() < 0.2}
    rows = [0 if r in exclusive else rng.randint(1, 5) for r in range(n)]
    lengths = [rng.choice([0, rng.randint(1, 40)]) if rng.random() < 0.15 else rng.randint(1, 40) for _ in range(sum(rows))]
    return dict(arrivals=arrivals, rows_per_request=rows, lengths=lengths, slots=slots, chunk=chunk, admit_min=admit_min,
                wave_hold=wave_hold, exclusive=exclusive)


def stream_case(seed, cfm=False):
    """-> (plan_online's keywords, the streaming requests {r: rows per fold}, the rows per fold of every request)"""
    rng = random.Random(seed)
    n = rng.randint(1, 8)
    slots, chunk = rng.randint(1, 8), rng.randint(1, 16)
    arrivals = [rng.randint(0, 12) for _ in range(n)]
    exclusive = {r for r in range(n) if rng.random() < 0.15}
    folds = [[rng.randint(1, 3) for _ in range(rng.randint(1, 4))] for _ in range(n)]       # rows per fold, every request
    rows = [0 if r in exclusive else sum(folds[r]) for r in range(n)]
    lengths = [rng.choice([0, rng.randint(1, 40)]) for _ in range(sum(rows))]
    streaming = {r: folds[r] for r in range(n) if rng.random() < 0.5}                   # may name exclusive requests too
    c = dict(arrivals=arrivals, rows_per_request=rows, lengths=lengths, slots=slots, chunk=chunk,
             admit_min=rng.choice([None, 1]), wave_hold=rng.choice([0, 1, 3]), exclusive=exclusive)
    if cfm:
        c.update(cfm_folds=[[[(rng.choice([1, 2, 4, 7]), rng.random() < 0.2) for _ in range(rng.choice([0, 1, 1, 2, 3]))] for _ in f]
                            for f in folds], cfm_rows=rng.randint(2, 6), cfm_chunk=rng.randint(1, 3))
    return c, streaming, folds


TRACE_SEEDS = range(200)
TRACE_VARIANTS = ("plain", "exclusive", "cfm_folds", "streaming", "cfm_folds+streaming")


def trace_case(seed, variant):
    """the keywords of the recorded plan_online trace of (seed, variant)"""
    if variant == "plain":
        return plan_case(seed, with_exclusive=False)
    if variant == "exclusive":
        return plan_case(seed)
    c, streaming, _ = stream_case(seed, cfm=variant.startswith("cfm_folds"))
    return dict(c, streaming=streaming) if variant.endswith("streaming") else c
