"""CPU: gsv.serving.plan_online, the schedule the serving Scheduler follows, as a pure function: properties over seeded random
arrival traces (slots 1-8, chunk 1-16, arrivals spread over 0-20 steps), and its equality with plan_continuous for a closed
queue."""
import pytest

from gsv.AR.models.t2s_model import plan_continuous
from gsv.serving import plan_online
from _serving_cases import plan_case as _case

CASES = 300


def _fifo(c):
    """(request, row) of every session row in queue order: arrival, then request number, then row"""
    order = sorted(range(len(c["arrivals"])), key=lambda r: (c["arrivals"][r], r))
    return [(r, k) for r in order if r not in c["exclusive"] for k in range(c["rows_per_request"][r])]


@pytest.mark.parametrize("seed", range(CASES))
def test_plan_online_properties(seed):
    c = _case(seed)
    trace = plan_online(**c, with_steps=True)
    assert [e for _, e in trace] == plan_online(**c)
    n = len(c["arrivals"])
    first = {}
    for r in range(n):
        first[r] = sum(c["rows_per_request"][:r])
    order = sorted(range(n), key=lambda r: (c["arrivals"][r], r))

    # every row is admitted exactly once, in FIFO order, never before its request arrived, into the lowest free slots
    admitted = [(r, k) for _, e in trace if e[0] == "admit" for r, k, _ in e[1]]
    assert admitted == _fifo(c)
    owner, left, finished_at, waved_at, served = {}, {}, {}, {}, []
    steps = [s for s, _ in trace]
    assert steps == sorted(steps)
    for step, e in trace:
        if e[0] == "admit":
            free = [s for s in range(c["slots"]) if s not in owner]
            assert [s for _, _, s in e[1]] == free[:len(e[1])], "rows go into the lowest free slots"
            for r, k, s in e[1]:
                assert step >= c["arrivals"][r]
                assert s not in owner, "a slot is reused only after the advance that reported its row"
                owner[s], left[s] = (r, k), c["lengths"][first[r] + k]
                # nothing later passes an exclusive request
                assert all(x in served for x in c["exclusive"] if order.index(x) < order.index(r))
        elif e[0] == "advance":
            assert e[1] == c["chunk"] and owner, "an advance needs a live row"
            done = []
            for s in sorted(owner):
                left[s] -= min(c["chunk"], left[s])
                if left[s] == 0:
                    done.append(owner[s])
            assert e[2] == done
            for s in [s for s in owner if owner[s] in done]:
                finished_at[owner.pop(s)] = step
        elif e[0] == "wave":
            for r in e[1]:
                assert r not in waved_at and r not in c["exclusive"]
                waved_at[r] = step
                back = [finished_at.get((r, k)) for k in range(c["rows_per_request"][r])]
                assert None not in back, "a request is in a wave only after all its rows finished"
                assert 0 <= step - max(back) <= c["wave_hold"], "and at most wave_hold steps later"
        elif e[0] == "exclusive":
            r = e[1]
            assert r in c["exclusive"] and r not in served and not owner, "an exclusive request runs when nothing is live"
            assert step >= c["arrivals"][r]
            # it passes nothing either: every earlier request has been admitted in full (and has finished: nothing is live)
            earlier = [x for x in order[:order.index(r)]]
            assert all(x in served if x in c["exclusive"] else (x, c["rows_per_request"][x] - 1) in finished_at for x in earlier)
            served.append(r)
        else:
            assert e == ("close",) and not owner
    assert sorted(waved_at) == [r for r in range(n) if r not in c["exclusive"]]
    assert sorted(served) == sorted(c["exclusive"])
    assert [r for r in order if r in c["exclusive"]] == served, "exclusive requests run in arrival order"
    assert trace[-1][1] == ("close",), "the trace ends with a close"
    # a session is closed before an exclusive request runs: between an admit and an exclusive there is a close
    open_ = False
    for _, e in trace:
        if e[0] == "admit":
            open_ = True
        elif e[0] == "close":
            open_ = False
        elif e[0] == "exclusive":
            assert not open_


@pytest.mark.parametrize("seed", range(CASES))
def test_a_closed_queue_is_plan_continuous(seed):
    c = _case(1000 + seed, closed=True)
    flat = _fifo(c)
    trace = plan_online(**c)
    got = []
    for e in trace:
        if e[0] == "admit":
            got.append(("admit", [(flat.index((r, k)), s) for r, k, s in e[1]]))
        elif e[0] == "advance":
            got.append(("advance", e[1], [flat.index(x) for x in e[2]]))
    assert got == plan_continuous(c["lengths"], c["slots"], c["chunk"], c["admit_min"])
    assert trace[-1] == ("close",) and sum(e == ("close",) for e in trace) == 1


def test_a_short_request_is_delivered_before_a_long_one_and_late_arrivals_take_free_slots():
    # request 0: one row of 40 steps; request 1: one row of 3; request 2 arrives at step 2 and takes request 1's slot
    trace = plan_online([0, 0, 2], [1, 1, 1], [40, 3, 5], slots=2, chunk=4, admit_min=1)
    assert trace[:3] == [("admit", [(0, 0, 0), (1, 0, 1)]), ("advance", 4, [(1, 0)]), ("wave", [1])]
    assert ("admit", [(2, 0, 1)]) in trace
    waves = [e[1] for e in trace if e[0] == "wave"]
    assert waves == [[1], [2], [0]]


def test_wave_hold_gathers_company_but_never_waits_on_an_idle_engine():
    kw = dict(arrivals=[0, 0, 0], rows_per_request=[1, 1, 1], lengths=[2, 4, 20], slots=3, chunk=2, admit_min=1)
    assert [e[1] for e in plan_online(**kw, wave_hold=0) if e[0] == "wave"] == [[0], [1], [2]]
    assert [e[1] for e in plan_online(**kw, wave_hold=1) if e[0] == "wave"] == [[0, 1], [2]]
    # the last request is alone: it is not held although wave_hold allows it
    t = plan_online(**kw, wave_hold=5, with_steps=True)
    last_adv = max(s for s, e in t if e[0] == "advance")
    assert [s for s, e in t if e[0] == "wave"][-1] == last_adv


def test_an_exclusive_request_is_a_barrier():
    trace = plan_online([0, 0, 0], [2, 0, 1], [5, 5, 5], slots=4, chunk=8, admit_min=1, exclusive=[1])
    assert trace == [("admit", [(0, 0, 0), (0, 1, 1)]), ("advance", 8, [(0, 0), (0, 1)]), ("wave", [0]), ("close",),
                     ("exclusive", 1), ("admit", [(2, 0, 0)]), ("advance", 8, [(2, 0)]), ("wave", [2]), ("close",)]


def test_bad_arguments():
    with pytest.raises(ValueError):
        plan_online([0], [1], [3], slots=0, chunk=4)
    with pytest.raises(ValueError):
        plan_online([0], [1], [3], slots=2, chunk=0)
    with pytest.raises(ValueError):
        plan_online([0], [2], [3], slots=2, chunk=4)
    with pytest.raises(ValueError):
        plan_online([0, 1], [1], [3], slots=2, chunk=4)
    with pytest.raises(ValueError):
        plan_online([0], [1], [3], slots=2, chunk=4, admit_min=0)
