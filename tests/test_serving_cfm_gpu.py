"""GPU: gsv.serving.Scheduler(continuous_cfm=True) on the fp32 small v3 / v4 pipelines of test_pipeline_v3_gpu.py: the waveform
stage as an open flow-matching session behind the decode session.  The requests are the mix of
test_run_batch_cfm_session_gpu.py (three voices; sample_steps 2 / 3 / 4; two guided requests at 0.7; one LoRA voice; one request
of two folds; one parallel_infer=False), arriving one and three scheduler steps apart, with cfm_rows = 8 below the mix's 30-odd DiT
rows so that slots are refilled.

The yardstick: a request's result is what run_batch([request]) returns for it alone -- the same AR tokens, int16 audio of the
same shape within BAR = 5e-3 of full scale, the bar test_run_batch_cfm_session_gpu.py holds the session path to against the
same yardstick."""
from concurrent.futures import CancelledError

import numpy as np
import pytest

from gsv.module.models import CFMSession
from gsv.serving import Scheduler, plan_online
from test_pipeline_v3_gpu import _build as build_v3
from test_run_batch_cfm_gpu import BAR, _diff, _spy as _cfm_calls
from test_run_batch_cfm_session_gpu import _mix
from test_run_batch_continuous_gpu import _run_batch
from test_run_batch_shared_gpu import _lsb
from test_serving_gpu import _run_to_idle, _spy

pytestmark = pytest.mark.gpu
WAIT = 120.0
CFM_ROWS = 8
SESSION = [0, 1, 2, 4, 5]                       # the requests that decode in the sessions; 3 is parallel_infer=False
SCHEDULE = [[0], [1], [], [], [2], [4], [], [], [5]]          # submitted in front of steps 0, 1, 4, 5, 8
# (rows, prompt lengths) of the inference_rows calls a Scheduler(chunk=8) without the keyword issues for SCHEDULE on the commit
# before the keyword existed, recorded there with _spy of test_run_batch_cfm_gpu.py
PARENT_CALLS = {"v3": [(6, [14]), (3, [14]), (11, [20]), (3, [17]), (7, [20])],
                "v4": [(6, [14]), (3, [14]), (11, [20]), (4, [17]), (7, [20])]}


@pytest.fixture(scope="module", params=["v3", "v4"])
def world(request):
    """the pipeline, the mix with its voices, per request what run_batch([request]) alone returns (sr, audio, tokens) and how
    many flow-matching rows it took there, and the inference_rows spy (which stays installed)"""
    version = request.param
    tts, _, (vcfg, vsd, _), _ = build_v3(version)
    batch = _mix(tts, version, vcfg, vsd)
    calls = _cfm_calls(tts)
    alone, rows = [], []
    for req in batch:
        del calls[:]
        out, preds = _run_batch(tts, [dict(req)], shared_cfm=True)
        rows.append(sum(n for n, _ in calls))
        plain = tts.run_batch([dict(req)])[0]
        assert _diff(plain[1], out[0][1]) <= BAR
        alone.append((plain[0], plain[1], preds[0]))
        assert np.abs(plain[1]).max() > 0
    return version, tts, batch, alone, rows, calls


def _check(world, r, result, seen, what):
    _, _, batch, alone, _, _ = world
    sr, audio, tokens = alone[r]
    assert not isinstance(result, BaseException), f"request {r} raised {result!r}"
    assert seen[batch[r]["seed"]][0] == tokens, f"request {r}: other AR tokens than in run_batch([request])"
    assert result[0] == sr and result[1].dtype == np.int16 and result[1].shape == audio.shape, f"request {r}: {result[1].shape} vs {audio.shape}"
    d = _diff(result[1], audio)
    print(f"{what}, request {r}: {_lsb(result[1], audio)} LSB = {d:.3e} of full scale from run_batch([request]) over {audio.size} samples")
    assert d <= BAR, f"request {r}: {d:.3e} of full scale"


def _serve(world, schedule, **kw):
    _, tts, batch, _, _, calls = world
    results, ticket_of = {}, {}
    del calls[:]
    with _spy(tts) as (seen, _), Scheduler(tts, chunk=8, **kw) as sched:
        for rs in schedule:
            for r in rs:
                ticket_of[r] = sched.submit(batch[r])
            results.update(sched.step())
        _run_to_idle(sched, results)
        assert sched._ses is None and sched._cfm is None, "an idle scheduler has closed both sessions"
    return {r: results[t] for r, t in ticket_of.items()}, ticket_of, seen, sched


def _plan_of(world, sched, ticket_of, seen, exclusive=()):
    """plan_online fed with the run's arrivals, its measured AR lengths and its rows per fold"""
    _, _, batch, _, _, _ = world
    by_ticket = sorted(ticket_of, key=lambda r: ticket_of[r])
    assert [ticket_of[r] for r in by_ticket] == list(range(len(by_ticket)))
    stats = sched.stats
    ex = [ticket_of[r] for r in exclusive]
    lengths = [n for r in by_ticket if r not in exclusive for idx in seen[batch[r]["seed"]][1] for n in idx]
    folds = [[] if r in exclusive else stats["cfm_folds"][ticket_of[r]] for r in by_ticket]
    return plan_online([stats["tickets"][t][0] for t in range(len(by_ticket))], [len(batch[r]["segments"]) for r in by_ticket], lengths,
                       slots=4, chunk=8, exclusive=ex, cfm_folds=folds, cfm_rows=sched._cpol.rows, cfm_chunk=sched._cpol.chunk)


@pytest.mark.parametrize("cfm_chunk", [1, 2])
def test_staggered_arrivals_through_both_sessions(world, cfm_chunk):
    version, tts, batch, alone, rows, calls = world
    results, ticket_of, seen, sched = _serve(world, SCHEDULE, continuous_cfm=True, cfm_rows=CFM_ROWS, cfm_chunk=cfm_chunk)
    for r in SESSION:
        _check(world, r, results[r], seen, f"{version} cfm_chunk {cfm_chunk}")
    stats, ev = sched.stats, sched.stats["events"]
    assert calls == [], f"no one-shot pass: {calls}"
    assert ev == _plan_of(world, sched, ticket_of, seen)
    assert all(e[0] != "wave" for e in ev) and stats["waves"] == 0
    # every request brought the rows its one-shot stage takes; request 2 two folds; 2 / 3 / 4 steps and both rates met in the session
    assert [sum(len(f) for f in stats["cfm_folds"][ticket_of[r]]) for r in SESSION] == [rows[r] for r in SESSION]
    assert len([f for f in stats["cfm_folds"][ticket_of[2]] if f]) == 2
    kinds = {row for t in stats["cfm_folds"].values() for f in t for row in f}
    assert {n for n, _ in kinds} == {2, 3, 4} and {g for _, g in kinds} == {False, True}
    admitted = [s for e in ev if e[0] == "cfm_admit" for _, _, _, s in e[1]]
    assert len(admitted) == sum(rows[r] for r in SESSION) == stats["cfm_rows"] > CFM_ROWS
    assert len(set(admitted)) < len(admitted), "a freed slot is given to a waiting row"
    assert max(stats["cfm_occupancy"]) <= CFM_ROWS and len(stats["cfm_occupancy"]) == sum(e[0] == "cfm_step" for e in ev)
    assert all(e[1] <= cfm_chunk for e in ev if e[0] == "cfm_step")
    assert stats["cfm_steps"] == sum(e[1] for e in ev if e[0] == "cfm_step")
    assert stats["cfm_admissions"] == sum(e[0] == "cfm_admit" for e in ev)
    assert stats["vocoder_calls"] == sum(len(e[1]) for e in ev if e[0] == "vocode") == 6      # one call per fold
    assert sorted(t for e in ev if e[0] == "deliver" for t in e[1]) == sorted(ticket_of.values())
    # a request is delivered while later ones are still in flight
    assert stats["tickets"][ticket_of[0]][2] < stats["tickets"][ticket_of[5]][2]


def test_shared_vocoder_takes_the_folds_of_a_step_in_one_pass(world):
    version, *_ = world
    results, ticket_of, seen, sched = _serve(world, [[0, 1, 2]], continuous_cfm=True, cfm_rows=32, cfm_chunk=2, shared_vocoder=True)
    for r in (0, 1, 2):
        _check(world, r, results[r], seen, f"{version} shared_vocoder")
    ev = sched.stats["events"]
    assert ev == _plan_of(world, sched, ticket_of, seen)
    assert sched.stats["vocoder_calls"] == sum(e[0] == "vocode" for e in ev) < sum(len(e[1]) for e in ev if e[0] == "vocode")


def test_cancel_with_live_flow_matching_rows(world):
    version, tts, batch, _, rows, _ = world
    results = {}
    with _spy(tts) as (seen, _), Scheduler(tts, chunk=8, continuous_cfm=True, cfm_rows=CFM_ROWS, cfm_chunk=1) as sched:
        t0, t2 = sched.submit(batch[0]), sched.submit(batch[2])
        n = 0
        while not any(o is not None and o[0] == t2 for o in sched._cpol.owner):
            results.update(sched.step())
            n += 1
            assert n <= 40, "request 2 never reaches the flow-matching session"
        held = [s for s, o in enumerate(sched._cpol.owner) if o is not None and o[0] == t2]
        assert held and sched.cancel(t2) and not sched.cancel(t2)
        assert sched.stats["events"][-1] == ("cfm_release", held) and sched.stats["cfm_released"] == len(held)
        state = sched._cfm.state
        assert all(state[s][0] == CFMSession.FREE for s in held)
        assert t2 not in sched._cfm_req and all(e[0] != t2 for e in sched._cpol.fifo)
        t5 = sched.submit(batch[5])
        _run_to_idle(sched, results)
        ev = sched.stats["events"]
    assert isinstance(results[t2], CancelledError)
    assert batch[2]["seed"] not in seen, "a cancelled request is not finished"
    _check(world, 0, results[t0], seen, f"{version} next to a cancelled request")
    _check(world, 5, results[t5], seen, f"{version} after a cancelled request")
    later = ev[ev.index(("cfm_release", held)) + 1:]
    again = {s for e in later if e[0] == "cfm_admit" for _, _, _, s in e[1]} & set(held)
    assert len(again) == min(len(held), rows[5]), "the released slots are admitted into again (request 5's rows, lowest slots first)"
    assert all(row[0] != t2 for e in later if e[0] in ("cfm_admit", "cfm_step") for row in e[-1])


def test_an_exclusive_request_in_the_middle(world):
    version, tts, batch, alone, _, calls = world
    results, ticket_of, seen, sched = _serve(world, [[0], [3], [4]], continuous_cfm=True, cfm_rows=CFM_ROWS, cfm_chunk=2)
    for r in (0, 4):
        _check(world, r, results[r], seen, f"{version} around an exclusive request")
    assert results[3][0] == alone[3][0] and np.array_equal(results[3][1], alone[3][1]), "run_batch([request]) itself: bit-equal"
    ev, stats = sched.stats["events"], sched.stats
    assert ev == _plan_of(world, sched, ticket_of, seen, exclusive=[3])
    i = ev.index(("exclusive", ticket_of[3]))
    assert ev[i - 1] == ("close",) and ("deliver", [ticket_of[0]]) in ev[:i]
    assert any(e[0] == "cfm_admit" for e in ev[:i]) and any(e[0] == "cfm_admit" for e in ev[i:])
    assert stats["sessions"] == 2 and stats["cfm_sessions"] == 2, "both sessions were closed before it and reopened after it"


def test_keyword_off_is_the_scheduler_as_it_was(world):
    version, tts, batch, _, _, calls = world
    opened = []
    inner = tts.vits_model.cfm.open_session
    tts.vits_model.cfm.open_session = lambda *a, **k: opened.append(a) or inner(*a, **k)
    try:
        results, ticket_of, seen, sched = _serve(world, SCHEDULE)
    finally:
        del tts.vits_model.cfm.open_session
    print(f"{version} inference_rows calls without the keyword: {calls}")
    assert opened == [] and sched._cpol is None and "cfm_steps" not in sched.stats
    assert calls == PARENT_CALLS[version], calls
    for r in SESSION:
        _check(world, r, results[r], seen, f"{version} keyword off")


def test_through_the_server(world):
    version, tts, batch, _, _, calls = world
    del calls[:]
    with _spy(tts) as (seen, threads):
        server = tts.serve(chunk=8, continuous_cfm=True, cfm_rows=CFM_ROWS, cfm_chunk=2)
        try:
            futures = {r: server.submit(batch[r]) for r in (0, 2, 4, 5)}
            server.cancel(futures[2])
            results = {r: f.result(timeout=WAIT) for r, f in futures.items() if r != 2}
            with pytest.raises(CancelledError):
                futures[2].result(timeout=WAIT)
        finally:
            server.shutdown(timeout=WAIT)
        assert not server._thread.is_alive() and server.error is None
        assert threads == {server._thread.ident}
    for r in (0, 4, 5):
        _check(world, r, results[r], seen, f"{version} Server")
    assert calls == [] and server.scheduler.stats["cfm_sessions"] >= 1
    out = tts.run_batch([dict(batch[0])])                            # both engines are handed back
    assert _diff(out[0][1], world[3][0][1]) == 0.0
