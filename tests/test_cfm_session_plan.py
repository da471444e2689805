"""CPU: plan_cfm_session, the pure schedule of a flow-matching session -- which rows are admitted before which step() call
and how many steps each call runs -- replayed here against the rules a session enforces.  No engine, no compute."""
import inspect
import random

import pytest

from gsv.TTS_infer_pack.TTS import TTS, plan_cfm_session


def _replay(rows, cap, schedule):
    """runs the schedule as a session would: -> (steps taken per row, admission order, live DiT rows at every step call,
    total DiT row-steps); asserts what the engine would refuse"""
    need = [2 if g else 1 for _, g in rows]
    taken, live, order, peaks, row_steps = [0] * len(rows), [], [], [], 0
    for admit, k in schedule:
        assert k >= 1
        for i in admit:
            free = cap - sum(need[j] for j in live)
            assert need[i] <= free, f"row {i} (needs {need[i]}) admitted into {free} free DiT rows"
            live.append(i)
            order.append(i)
        assert live, "a step() call without a live row"
        peaks.append(sum(need[j] for j in live))
        assert k == min(rows[j][0] - taken[j] for j in live), "a call runs until the next row finishes, no further"
        for j in live:
            taken[j] += k
            row_steps += k * need[j]
        live = [j for j in live if taken[j] < rows[j][0]]
    assert not live
    return taken, order, peaks, row_steps


CASES = {
    "thirds": ([(s, False) for s in (8, 16, 32) * 4], 6),
    "guided_mix": ([(4, True), (2, False), (3, True), (8, False), (1, True), (5, False), (2, True)], 4),
    "guided_head_waits": ([(3, False), (2, False), (4, False), (5, True), (1, False)], 3),
    "cap_1": ([(2, False), (1, False), (3, False)], 1),
    "all_guided_cap_3": ([(2, True), (3, True), (1, True)], 3),      # the third DiT row is never usable
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_schedule_obeys_the_session_rules(name):
    rows, cap = CASES[name]
    sched = plan_cfm_session(rows, cap)
    taken, order, peaks, row_steps = _replay(rows, cap, sched)
    assert taken == [s for s, _ in rows], "every row gets exactly its step count"
    assert order == list(range(len(rows))), "admission is FIFO"
    assert max(peaks) <= cap, "the live DiT rows never exceed the cap"
    assert row_steps == sum(s * (2 if g else 1) for s, g in rows), "row-steps = the step counts, plus the twins'"


def test_random_inputs():
    rng = random.Random(7)
    for _ in range(200):
        cap = rng.randint(2, 9)
        rows = [(rng.choice((1, 2, 3, 4, 8, 16, 32)), rng.random() < 0.4) for _ in range(rng.randint(1, 30))]
        taken, order, peaks, row_steps = _replay(rows, cap, plan_cfm_session(rows, cap))
        assert taken == [s for s, _ in rows] and order == list(range(len(rows))) and max(peaks) <= cap
        assert row_steps == sum(s * (2 if g else 1) for s, g in rows)


def test_a_guided_row_is_never_admitted_into_one_free_dit_row():
    """cap 3: after the first call two unguided rows are live and one DiT row is free, with a guided row at the head of the
    queue: it waits, and the unguided row behind it does not overtake it"""
    rows = [(3, False), (3, False), (2, False), (4, True), (1, False)]
    sched = plan_cfm_session(rows, 3)
    assert sched[0] == ([0, 1, 2], 2)
    assert sched[1] == ([], 1), "row 2 has left, one DiT row is free: nobody is admitted"
    assert sched[2] == ([3, 4], 1)
    _replay(rows, 3, sched)


def test_uniform_input_within_the_cap_is_one_admission_and_one_step_call():
    assert plan_cfm_session([(32, False)] * 8, 8) == [(list(range(8)), 32)]
    assert plan_cfm_session([(5, True)] * 4, 8) == [(list(range(4)), 5)]
    assert plan_cfm_session([(5, True)] * 4, 32) == [(list(range(4)), 5)]


def test_empty_input_and_bad_input():
    assert plan_cfm_session([], 4) == []
    with pytest.raises(ValueError):
        plan_cfm_session([(2, True)], 1)
    with pytest.raises(ValueError):
        plan_cfm_session([(0, False)], 4)


def test_keyword_defaults():
    assert inspect.signature(TTS.run_batch).parameters["continuous_cfm"].default is False
    assert inspect.signature(TTS._shared_cfm_stage).parameters["continuous_cfm"].default is False
