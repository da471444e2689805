"""CPU: gsv.serving.plan_online with the flow-matching inputs (cfm_folds, cfm_rows, cfm_chunk) -- the schedule of
Scheduler(continuous_cfm=True) as a pure function -- and the keyword's defaults and refusals on a stub pipeline."""
import inspect
import types

import pytest

from gsv.serving import Scheduler, plan_online
from _serving_cases import plan_case as _case

CASES = 300

U, G = False, True


def _plan(arrivals, folds, ar_lengths=None, slots=8, chunk=8, cfm_rows=4, cfm_chunk=2, exclusive=(), **kw):
    """every request brings one AR row per fold-row count given in `ar_rows` (default 1) that ends at its admission"""
    rows = [0 if r in exclusive else 1 for r in range(len(arrivals))]
    lengths = ar_lengths if ar_lengths is not None else [0] * sum(rows)
    return plan_online(arrivals, rows, lengths, slots=slots, chunk=chunk, admit_min=1, exclusive=exclusive, cfm_folds=folds,
                       cfm_rows=cfm_rows, cfm_chunk=cfm_chunk, **kw)


def _of(trace, kind):
    return [e for e in trace if e[0] == kind]


def test_fifo_order_and_lowest_slot_admission():
    # request 0: two folds of 2 and 1 rows, 4 steps; request 1 (same step): one fold of 2 rows, 2 steps.  cfm_rows = 4
    trace = _plan([0, 0], [[[(4, U)] * 2, [(4, U)]], [[(2, U)] * 2]])
    assert "wave" not in [e[0] for e in trace]
    admits = _of(trace, "cfm_admit")
    # (arrival, bi, k) order into slots 0 .. 3; request 1's second row waits for a slot
    assert admits[0] == ("cfm_admit", [(0, 0, 0, 0), (0, 0, 1, 1), (0, 1, 0, 2), (1, 0, 0, 3)])
    # step 0: k = 2; request 1's row (2 steps) finishes, its slot 3 -- the lowest free one -- goes to the waiting row
    assert _of(trace, "cfm_step")[0] == ("cfm_step", 2, [(1, 0, 0)])
    assert admits[1] == ("cfm_admit", [(1, 0, 1, 3)])
    # step 1: request 0's rows finish (4 steps), both its folds are vocoded in one event, and it is delivered
    assert _of(trace, "cfm_step")[1] == ("cfm_step", 2, [(0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 1)])
    assert _of(trace, "vocode") == [("vocode", [(0, 0), (0, 1), (1, 0)])]
    assert _of(trace, "deliver") == [("deliver", [0, 1])]
    assert trace[-1] == ("close",) and trace.count(("close",)) == 1


def test_a_guided_row_counts_two():
    trace = _plan([0], [[[(2, G), (2, G), (2, U)]]], cfm_rows=4)
    admits = _of(trace, "cfm_admit")
    assert admits[0] == ("cfm_admit", [(0, 0, 0, 0), (0, 0, 1, 1)])          # 2 + 2 DiT rows; the unguided row waits
    assert admits[1] == ("cfm_admit", [(0, 0, 2, 0)])
    # cfm_rows = 1 is raised to 2 for a guided row, which then runs alone
    trace = _plan([0], [[[(1, U), (1, G), (1, U)]]], cfm_rows=1, cfm_chunk=4)
    assert [e[1] for e in _of(trace, "cfm_admit")] == [[(0, 0, 0, 0)], [(0, 0, 1, 0)], [(0, 0, 2, 0)]]
    trace = _plan([0], [[[(1, G), (1, U), (1, U)]]], cfm_rows=1, cfm_chunk=4)
    assert [e[1] for e in _of(trace, "cfm_admit")] == [[(0, 0, 0, 0)], [(0, 0, 1, 0), (0, 0, 2, 1)]]


def test_head_of_line_blocking_at_cfm_rows_and_at_nine_step_counts():
    # the guided head does not fit 3 DiT rows next to two live rows; the unguided row behind it would, and is not taken
    trace = _plan([0], [[[(3, U), (3, U), (1, G), (1, U)]]], cfm_rows=3, cfm_chunk=8)
    # (both live rows leave together after 3 steps: slots 0 and 1 are free again, and are taken in that order)
    assert [e[1] for e in _of(trace, "cfm_admit")] == [[(0, 0, 0, 0), (0, 0, 1, 1)], [(0, 0, 2, 0), (0, 0, 3, 1)]]
    assert [e[1:] for e in _of(trace, "cfm_step")][0] == (3, [(0, 0, 0), (0, 0, 1)])
    # nine rows with nine step counts, sixteen DiT rows: eight tables at most, the ninth row waits for a row to leave
    folds = [[[(n, U)] for n in range(2, 11)]]
    trace = _plan([0], folds, cfm_rows=16, cfm_chunk=16)
    admits = _of(trace, "cfm_admit")
    assert [len(e[1]) for e in admits] == [8, 1]
    assert admits[1][1] == [(0, 8, 0, 0)]                                       # the slot of the 2-step row
    # with eight distinct counts nothing waits
    assert [len(e[1]) for e in _of(_plan([0], [[[(2 + n % 8, U)] for n in range(9)]], cfm_rows=16), "cfm_admit")] == [9]


def test_k_is_the_smaller_of_cfm_chunk_and_the_least_remaining():
    trace = _plan([0], [[[(5, U), (3, U), (8, U)]]], cfm_rows=4, cfm_chunk=2)
    assert [(e[1], e[2]) for e in _of(trace, "cfm_step")] == [(2, []), (1, [(0, 0, 1)]), (2, [(0, 0, 0)]), (2, []), (1, [(0, 0, 2)])]
    trace = _plan([0], [[[(5, U), (3, U), (8, U)]]], cfm_rows=4, cfm_chunk=16)
    assert [e[1] for e in _of(trace, "cfm_step")] == [3, 2, 3]
    # one scheduler step never runs more than cfm_chunk Euler steps, and takes arrivals in before the next
    trace = _plan([0, 1], [[[(6, U)]], [[(2, U)]]], cfm_rows=4, cfm_chunk=2, with_steps=True)
    assert [(s, e[1]) for s, e in trace if e[0] == "cfm_step"] == [(0, 2), (1, 2), (2, 2)]
    assert (1, ("cfm_admit", [(1, 0, 0, 1)])) in trace
    # the late, short request is fetched, vocoded and delivered in the step it finishes, one step before the long one
    assert [(s, e) for s, e in trace if e[0] in ("vocode", "deliver")] == [
        (1, ("vocode", [(1, 0)])), (1, ("deliver", [1])), (2, ("vocode", [(0, 0)])), (2, ("deliver", [0]))]


def test_a_fold_spanning_two_admissions_is_vocoded_once():
    trace = _plan([0], [[[(2, U)] * 3]], cfm_rows=2, cfm_chunk=2)
    assert [len(e[1]) for e in _of(trace, "cfm_admit")] == [2, 1]
    assert _of(trace, "vocode") == [("vocode", [(0, 0)])]
    assert trace.index(("vocode", [(0, 0)])) == trace.index(("cfm_step", 2, [(0, 0, 2)])) + 1, "after its last row came back"
    assert _of(trace, "deliver") == [("deliver", [0])]


def test_an_exclusive_request_waits_for_both_sessions_and_closes_both():
    # request 0 decodes (AR: one row that ends at once) and needs 3 scheduler steps of flow matching; request 1, exclusive,
    # arrives in step 1; request 2 arrives in step 1 too and stays behind the barrier
    trace = _plan([0, 1, 1], [[[(6, U)]], [], [[(2, U)]]], ar_lengths=[0, 0], exclusive=[1], cfm_chunk=2, with_steps=True)
    ev = [e for _, e in trace]
    i_ex = ev.index(("exclusive", 1))
    assert ev[i_ex - 1] == ("close",), "both sessions are closed in front of it"
    assert ev.index(("deliver", [0])) < i_ex, "it waits for the flow-matching rows that are live"
    assert [s for s, e in trace if e == ("exclusive", 1)] == [2]
    assert all(e[0] != "admit" or e[1][0][0] != 2 for e in ev[:i_ex]), "nothing passes the barrier"
    assert ev[i_ex + 1:] == [("admit", [(2, 0, 0)]), ("advance", 8, [(2, 0)]), ("cfm_admit", [(2, 0, 0, 0)]),
                             ("cfm_step", 2, [(2, 0, 0)]), ("vocode", [(2, 0)]), ("deliver", [2]), ("close",)]


def test_a_request_without_rows_is_delivered_in_its_step():
    # request 0 has no sentence (no AR row), request 1 has one sentence whose fold has no frames
    trace = plan_online([0, 0], [0, 1], [0], slots=2, chunk=4, admit_min=1, cfm_folds=[[], [[]]], cfm_rows=2, cfm_chunk=2,
                        with_steps=True)
    assert trace == [(0, ("admit", [(1, 0, 0)])), (0, ("advance", 4, [(1, 0)])), (0, ("deliver", [0, 1])), (0, ("close",))]


@pytest.mark.parametrize("seed", range(0, CASES, 3))
def test_without_the_new_inputs_the_trace_is_todays(seed):
    """the cases of test_serving_plan.py: the AR events of a trace with flow-matching rows are the AR events of the trace
    without, and the trace without is the reference trace that file pins (its properties hold there)"""
    c = _case(seed)
    plain = plan_online(**c)
    assert plain == plan_online(**c, cfm_folds=None, cfm_rows=None, cfm_chunk=None)
    assert all(e[0] in ("admit", "advance", "wave", "exclusive", "close") for e in plain)
    # wave_hold = 0, rows that need no flow matching: the delivery of a request replaces its wave, event for event
    c0 = dict(c, wave_hold=0)
    folds = [[] for _ in c["arrivals"]]
    with_cfm = plan_online(**c0, cfm_folds=folds, cfm_rows=4, cfm_chunk=2)
    assert [("wave", e[1]) if e[0] == "deliver" else e for e in with_cfm] == plan_online(**c0)


def test_bad_arguments():
    with pytest.raises(ValueError):
        plan_online([0], [1], [0], slots=2, chunk=4, cfm_folds=[[[(2, U)]]])                  # no cfm_rows / cfm_chunk
    with pytest.raises(ValueError):
        plan_online([0], [1], [0], slots=2, chunk=4, cfm_folds=[[[(2, U)]]], cfm_rows=0, cfm_chunk=1)
    with pytest.raises(ValueError):
        plan_online([0], [1], [0], slots=2, chunk=4, cfm_folds=[[[(2, U)]]], cfm_rows=2, cfm_chunk=0)
    with pytest.raises(ValueError):
        plan_online([0], [1], [0], slots=2, chunk=4, cfm_folds=[[[(0, U)]]], cfm_rows=2, cfm_chunk=1)
    with pytest.raises(ValueError):
        plan_online([0, 0], [1, 1], [0, 0], slots=2, chunk=4, cfm_folds=[[[(2, U)]]], cfm_rows=2, cfm_chunk=1)


def _stub(use_vocoder):
    return types.SimpleNamespace(t2s_model=types.SimpleNamespace(max_batch=8), vits_model=object(), cfm_max_rows=32,
                                 configs=types.SimpleNamespace(use_vocoder=use_vocoder))


def test_keyword_defaults_and_refusal_on_a_model_without_a_vocoder():
    sig = inspect.signature(Scheduler.__init__).parameters
    assert sig["continuous_cfm"].default is False and sig["cfm_rows"].default is None and sig["cfm_chunk"].default >= 1
    with pytest.raises(ValueError, match="vocoder"):
        Scheduler(_stub(False), continuous_cfm=True)
    off = Scheduler(_stub(False))                      # v2 without the keyword: as before
    assert off._cpol is None and "cfm_steps" not in off.stats
    on = Scheduler(_stub(True), continuous_cfm=True)
    assert on._cpol.rows == 32 and on._cpol.chunk == sig["cfm_chunk"].default      # min(cfm_max_rows, 64)
    big = _stub(True)
    big.cfm_max_rows = 200
    assert Scheduler(big, continuous_cfm=True)._cpol.rows == 64
    assert Scheduler(_stub(True), continuous_cfm=True, cfm_rows=5, cfm_chunk=3)._cpol.rows == 5
    with pytest.raises(ValueError):
        Scheduler(_stub(True), continuous_cfm=True, cfm_rows=65)
    with pytest.raises(ValueError):
        Scheduler(_stub(True), continuous_cfm=True, cfm_chunk=0)
