"""CPU: the scheduling of the AR decode sessions (continuous batching) as pure functions -- plan_continuous / admit_count of
gsv/AR/models/t2s_model.py on made-up lengths, and TTS.plan_sessions, the group-to-session mapping of
run_batch(continuous_ar=True), on stub plans."""
import random
import types

import pytest
import torch

from gsv.AR.models.t2s_model import admit_count, plan_continuous

CASES = [(slots, chunk, admit_min, n, seed) for slots in (1, 4, 32) for chunk in (1, 5, 16) for admit_min in (None, 1, 3)
         for n, seed in ((0, 0), (3, 1), (13, 2), (70, 3)) if admit_min is None or admit_min <= slots]


def _lengths(n, seed):
    rnd = random.Random(seed)
    return [rnd.choice((0, 1, 7, 16, 40, 41, 100)) for _ in range(n)]


@pytest.mark.parametrize("slots,chunk,admit_min,n,seed", CASES)
def test_schedule_invariants(slots, chunk, admit_min, n, seed):
    lengths = _lengths(n, seed)
    amin = max(1, slots // 4) if admit_min is None else admit_min
    trace = plan_continuous(lengths, slots, chunk, admit_min)
    owner = [None] * slots
    admitted, finished, ran = [], [], {}
    for k, ev in enumerate(trace):
        if ev[0] == "admit":
            pairs = ev[1]
            assert pairs, "an admission admits something"
            free_before = owner.count(None)
            queued = n - len(admitted)
            # admit_min is respected, except at the queue's tail and when nothing is decoding
            assert free_before >= min(amin, queued) or free_before == slots
            assert len(pairs) == min(free_before, queued), "an admission fills what is free"
            for row, s in pairs:
                assert owner[s] is None, f"row {row} admitted into live slot {s}"
                owner[s] = row
                ran[row] = 0
                admitted.append(row)
            assert len({s for _, s in pairs}) == len(pairs)
        else:
            assert ev[1] == chunk
            for s in range(slots):
                if owner[s] is not None:
                    ran[owner[s]] += chunk
            for row in ev[2]:
                s = owner.index(row)
                need = max(lengths[row], 1)        # a row that ends at its admission is reported by the next advance
                assert need <= ran[row] < need + chunk, "a row is reported by the advance in which it ends"
                owner[s] = None
                finished.append(row)
            assert all(ran[r] < lengths[r] for r in owner if r is not None), "a finished row does not keep its slot"
        assert sum(o is not None for o in owner) <= slots
    assert admitted == list(range(n)), "every row is admitted exactly once, in the order given"
    assert sorted(finished) == list(range(n))
    assert owner == [None] * slots


def test_queue_shorter_than_slots_is_one_static_batch():
    lengths = [30, 12, 0, 25]
    trace = plan_continuous(lengths, slots=8, chunk=10, admit_min=2)
    assert [ev[0] for ev in trace] == ["admit", "advance", "advance", "advance"]
    assert trace[0][1] == [(0, 0), (1, 1), (2, 2), (3, 3)]
    assert [ev[2] for ev in trace[1:]] == [[2], [1], [0, 3]]


def test_rows_wait_for_admit_min_free_slots():
    # 4 slots, admit_min 2: when row 0 ends after the first chunk one slot is free and the queue waits for a second one
    trace = plan_continuous([5, 10, 20, 20, 3, 3, 3], slots=4, chunk=5, admit_min=2)
    assert trace[0] == ("admit", [(0, 0), (1, 1), (2, 2), (3, 3)])
    assert trace[1] == ("advance", 5, [0]) and trace[2] == ("advance", 5, [1])
    assert trace[3] == ("admit", [(4, 0), (5, 1)])
    # the tail: one row left, it goes into the first slot that frees
    assert trace[4] == ("advance", 5, [4, 5]) and trace[5] == ("admit", [(6, 0)])


def test_admit_count():
    assert admit_count(free=0, queued=5, live=4, admit_min=1) == 0
    assert admit_count(free=3, queued=0, live=1, admit_min=1) == 0
    assert admit_count(free=1, queued=5, live=3, admit_min=2) == 0
    assert admit_count(free=2, queued=5, live=2, admit_min=2) == 2
    assert admit_count(free=1, queued=1, live=3, admit_min=2) == 1      # tail of the queue
    assert admit_count(free=4, queued=9, live=0, admit_min=8) == 4      # nothing decoding: never starve
    with pytest.raises(ValueError):
        plan_continuous([1], slots=0, chunk=4)
    with pytest.raises(ValueError):
        plan_continuous([1], slots=4, chunk=4, admit_min=0)


# ---- run_batch(continuous_ar=True): plan_batch's groups -> sessions ----

def _stub_tts(max_batch, max_seq=1000):
    from gsv.TTS_infer_pack.TTS import TTS
    t = TTS.__new__(TTS)
    t.t2s_model = types.SimpleNamespace(max_batch=max_batch, max_seq=max_seq)
    t.configs = types.SimpleNamespace(hz=50, max_sec=10)
    return t


def _stub_plans():
    def plan(seed, lens_per_batch, P, top_k, parallel=True, no_prompt=False):
        data = [dict(all_phones=[torch.zeros(n, dtype=torch.long) for n in lens]) for lens in lens_per_batch]
        opts = dict(top_k=top_k, top_p=1.0, temperature=1.0, repetition_penalty=1.35, parallel_infer=parallel)
        return dict(data=data, no_prompt=no_prompt, actual_seed=seed, opts=opts, P=P)
    return [plan(100, [[30, 12, 50], [8]], 40, 15), plan(200, [[20, 21, 22, 23, 24]], 77, 15), plan(300, [[9, 40]], 10, 5),
            plan(400, [[11, 12]], 0, 15, no_prompt=True), plan(500, [[13]], 33, 15, parallel=False)]


@pytest.mark.parametrize("mixed", [False, True])
def test_groups_become_sessions_with_plan_batch_keys(mixed):
    tts = _stub_tts(max_batch=4)
    plans = _stub_plans()
    launches = tts.plan_batch(plans, mixed_sampling=mixed)
    work = tts.plan_sessions(launches)
    # nothing is lost, nothing is changed: the same row dicts, in plan_batch's order
    assert [id(e) for _, rows in work for e in rows] == [id(e) for rows in launches for e in rows]
    sessions = [rows for s, rows in work if s]
    others = [rows for s, rows in work if not s]
    # one session per parallel-decode group with prompts, however many launches of max_batch it was cut into
    groups = {e["group"] for rows in launches for e in rows if e["group"][4] and not e["group"][5]}
    assert len(sessions) == len(groups) == (1 if mixed else 2)
    assert max(len(rows) for rows in sessions) > tts.t2s_model.max_batch, "the stub queue must exceed the slots"
    for rows in sessions:
        assert len({e["group"] for e in rows}) == 1
        assert [e["len"] for e in rows] == sorted(e["len"] for e in rows)
        for e in rows:
            pl = plans[e["r"]]
            assert e["key"] == (pl["actual_seed"] + e["bi"], e["j"] % 4)
            if mixed:
                o = pl["opts"]
                assert e["sampling"] == (o["top_k"], o["top_p"], o["temperature"], o["repetition_penalty"])
    # prompt-free and naive groups keep today's launches
    assert others == [rows for rows in launches if not (rows[0]["group"][4] and not rows[0]["group"][5])]
    assert all(len(rows) <= 4 for rows in others)
