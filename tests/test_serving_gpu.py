"""GPU: gsv.serving.Scheduler / Server on the fp32 small v2 pipeline of test_run_batch_gpu.py (max_batch 4, max_seq 256) with the
requests of test_run_batch_continuous_gpu.py (6 requests, 3 voices, 19 sentences, two sampling settings), chunk = 8.

The yardstick: a request's result through the scheduler is what run_batch([request]) gives for it alone on the same pipeline,
with no keywords -- the same AR token ids per sentence, audio of the same shape within 1 int16 LSB (the project's bar for
run_batch against run) -- whatever else is in flight, whatever the arrival order, whichever slot a row lands in."""
import contextlib
import threading
from concurrent.futures import CancelledError

import numpy as np
import pytest

from gsv.serving import Scheduler, plan_online
from test_run_batch_continuous_gpu import _requests, _run_batch
from test_run_batch_gpu import _build, _segs, _voice_args
from test_run_batch_shared_gpu import BASE, _lsb

pytestmark = pytest.mark.gpu

WAIT = 120.0


@pytest.fixture(scope="module")
def tts():
    return _build("v2")


@pytest.fixture(scope="module")
def world(tts):
    """the requests with their voices filled in, and for each what run_batch([request]) alone returns: (sr, audio, tokens)"""
    reqs = _requests(mixed=True)
    vfree = _voice_args(3, 5, 0, "v2", prompt_free=True)
    reqs.append((reqs[1][0], dict(BASE, segments=_segs(36, [7, 9, 5]), batch_size=2, seed=9, parallel_infer=False)))   # 6: naive loop
    reqs.append((vfree, dict(BASE, segments=_segs(37, [6, 8]), batch_size=2, seed=10)))                                # 7: prompt-free
    voices = {}
    for kw, _ in reqs:
        voices.setdefault(id(kw), tts.make_voice(**kw))
    batch = [dict(req, voice=voices[id(kw)]) for kw, req in reqs]
    assert len({r["seed"] for r in batch}) == len(batch)
    alone = []
    for req in batch:
        out, preds = _run_batch(tts, [req])
        alone.append((out[0][0], out[0][1], preds[0]))
        assert np.abs(out[0][1]).max() > 0
    assert sum(len(r["segments"]) for r in batch[:6]) == 19
    return batch, alone


@contextlib.contextmanager
def _spy(tts):
    """what every finished request decoded, by its seed: (tokens[bi][j], idx[bi][j]); and the threads that finished them"""
    seen, threads = {}, set()
    inner = tts._finish_request

    def spy(pl, sr):
        seen[pl["actual_seed"]] = ([[p.cpu().tolist() for p in pred] for pred in pl["preds"]],
                                   [[int(i) for i in idx] for idx in pl["idxs"]])
        threads.add(threading.get_ident())
        return inner(pl, sr)
    tts._finish_request = spy
    try:
        yield seen, threads
    finally:
        del tts._finish_request


def _meets_the_yardstick(world, r, result, seen):
    batch, alone = world
    sr, audio, tokens = alone[r]
    assert not isinstance(result, BaseException), f"request {r} raised {result!r}"
    assert seen[batch[r]["seed"]][0] == tokens, f"request {r}: a sentence decodes other tokens than in run_batch([request])"
    assert result[0] == sr and result[1].dtype == np.int16 and result[1].shape == audio.shape
    assert _lsb(result[1], audio) <= 1, f"request {r}: {_lsb(result[1], audio)} LSB from run_batch([request])"


def _run_to_idle(sched, results, limit=80):
    n = 0
    while not sched.idle:
        results.update(sched.step())
        n += 1
        assert n <= limit, "the scheduler does not come to rest"


def _serve(tts, world, schedule, **kw):
    """schedule[s]: the requests submitted in front of step s; then steps until idle.  -> results by request, what _spy saw,
    the (closed) scheduler"""
    batch = world[0]
    results, ticket_of = {}, {}
    with _spy(tts) as (seen, _), Scheduler(tts, chunk=8, **kw) as sched:
        for rs in schedule:
            for r in rs:
                ticket_of[r] = sched.submit(batch[r])
            results.update(sched.step())
        _run_to_idle(sched, results)
        assert sched._ses is None, "an idle scheduler has closed its session"
    return {r: results[t] for r, t in ticket_of.items()}, seen, sched


def test_staggered_arrival(tts, world):
    batch = world[0]
    results, ticket_of, submitted_last_at = {}, {}, None
    with _spy(tts) as (seen, _), Scheduler(tts, chunk=8) as sched:
        todo = [[0, 1], [2], [3], [4]]
        while todo or 5 not in ticket_of or not sched.idle:
            if todo:
                for r in todo.pop(0):
                    ticket_of[r] = sched.submit(batch[r])
            elif 5 not in ticket_of and results:          # the step after the first result came back
                ticket_of[5] = sched.submit(batch[5])
                submitted_last_at = sched.stats["steps"]
            results.update(sched.step())
            assert sched.stats["steps"] <= 80
        stats, sessions = sched.stats, sched.sessions
    assert sorted(results) == sorted(ticket_of.values())
    for r, t in ticket_of.items():
        _meets_the_yardstick(world, r, results[t], seen)
    delivered = {r: stats["tickets"][t][2] for r, t in ticket_of.items()}
    assert min(delivered.values()) < submitted_last_at == stats["tickets"][ticket_of[5]][0], \
        "a result must be delivered before the last request is even submitted"
    assert all(stats["tickets"][t][0] <= stats["tickets"][t][1] <= stats["tickets"][t][2] for t in ticket_of.values())
    # one session for the whole burst: 19 rows on 4 slots
    assert len(sessions) == 1 and stats["sessions"] == 1 and sessions[0].slots == 4
    assert len(sessions[0].history) == 19 and {s for _, s in sessions[0].history} == {0, 1, 2, 3}
    assert stats["rows"] == 19 and stats["admissions"] == len(sessions[0].adopt) >= 4
    assert max(stats["occupancy"]) == 4 and stats["advances"] == len(stats["occupancy"])
    # the recorded events are plan_online's, fed with the arrivals and the measured lengths (tickets are 0 .. 5 in request order)
    assert [ticket_of[r] for r in range(6)] == list(range(6))
    lengths = [n for r in range(6) for idx in seen[batch[r]["seed"]][1] for n in idx]
    assert len(lengths) == 19
    plan = plan_online([stats["tickets"][t][0] for t in range(6)], [len(batch[r]["segments"]) for r in range(6)], lengths,
                       slots=4, chunk=8)
    assert stats["events"] == plan
    assert stats["waves"] == sum(e[0] == "wave" for e in plan) and plan[-1] == ("close",)




def test_another_arrival_schedule_gives_the_same_tokens(tts, world):
    batch = world[0]
    a, seen_a, sched_a = _serve(tts, world, [[0, 1, 2, 3, 4, 5]])
    b, seen_b, sched = _serve(tts, world, [[5], [4], [3], [2], [1], [0]], admit_min=2, wave_hold=1)
    for r in range(6):
        _meets_the_yardstick(world, r, a[r], seen_a)
        _meets_the_yardstick(world, r, b[r], seen_b)
        assert seen_a[batch[r]["seed"]] == seen_b[batch[r]["seed"]], f"request {r}: the arrival order changes its tokens"
    assert sched.stats["rows"] == 19
    # not vacuous: the first rows admitted were request 0's in one schedule and request 5's (ticket 0 there) in the other
    first_a, first_b = ([e for e in s.stats["events"] if e[0] == "admit"][0][1] for s in (sched_a, sched))
    assert [t for t, _, _ in first_a] == [0, 0, 1, 1] and [t for t, _, _ in first_b] == [0, 0, 0]


def test_cancel_releases_the_live_rows(tts, world):
    batch = world[0]
    results = {}
    with _spy(tts) as (seen, _), Scheduler(tts, chunk=8) as sched:
        t0, t3 = sched.submit(batch[0]), sched.submit(batch[3])      # 2 + 4 rows on 4 slots: two rows of request 3 are live
        results.update(sched.step())
        assert sched.stats["events"][0] == ("admit", [(t0, 0, 0), (t0, 1, 1), (t3, 0, 2), (t3, 1, 3)])
        assert sched.stats["events"][1] == ("advance", 8, []), "the rows must still be decoding when the request is cancelled"
        assert sched.cancel(t3) and not sched.cancel(t3)
        assert sched.stats["released"] == 2 and sched.stats["events"][-1] == ("release", [2, 3])
        assert sched._ses.state()[1].tolist() == [1, 1, 0, 0]
        others = {r: sched.submit(batch[r]) for r in (1, 2, 4, 5)}
        _run_to_idle(sched, results)
        events, sessions = sched.stats["events"], sched.sessions
    assert isinstance(results[t3], CancelledError)
    others[0] = t0
    for r, t in others.items():
        _meets_the_yardstick(world, r, results[t], seen)
    assert batch[3]["seed"] not in seen, "a cancelled request must not reach the waveform stage"
    later = events[events.index(("release", [2, 3])) + 1:]
    assert {2, 3} <= {s for e in later if e[0] == "admit" for _, _, s in e[1]}, "the released slots are admitted again"
    assert all(row[0] != t3 for e in later if e[0] in ("admit", "advance") for row in e[-1])
    assert len(sessions) == 1 and len(sessions[0].history) == 2 + 2 + 13


def test_exclusive_requests_between_session_requests(tts, world):
    batch = world[0]
    order = [0, 6, 2, 7, 4]                    # 6: parallel_infer=False, 7: prompt-free -> tickets 1 and 3
    results, seen, sched = _serve(tts, world, [order])
    for r in order:
        _meets_the_yardstick(world, r, results[r], seen)
    events, stats = sched.stats["events"], sched.stats
    lengths = [n for r in (0, 2, 4) for idx in seen[batch[r]["seed"]][1] for n in idx]
    assert events == plan_online([0] * 5, [2, 0, 5, 0, 2], lengths, slots=4, chunk=8, exclusive=[1, 3])
    # the session is closed in front of each exclusive request and opened again by the next session row
    kinds = [e[0] for e in events if e[0] in ("admit", "close", "exclusive")]
    assert [k for k in kinds if k != "admit"] == ["close", "exclusive", "close", "exclusive", "close"]
    assert kinds[0] == "admit" and all(kinds[i + 1] == "admit" for i, k in enumerate(kinds) if k == "exclusive")
    assert [e[1] for e in events if e[0] == "exclusive"] == [1, 3]
    assert stats["sessions"] == 3 == len(sched.sessions) and stats["exclusive"] == 2
    assert [len(s.history) for s in sched.sessions] == [2, 5, 2]


def test_a_request_whose_planning_raises_gets_its_exception(tts, world):
    batch = world[0]
    unknown = dict(batch[1], lora_voice="nobody", seed=21)
    bad_ref = dict(BASE, segments=_segs(38, [6]), seed=22, ref_audio_path="no/such/reference.wav", prompt_text="x", prompt_lang="zh")
    results = {}
    with _spy(tts) as (seen, _), Scheduler(tts, chunk=8) as sched:
        tickets = [sched.submit(r) for r in (batch[0], unknown, batch[4], bad_ref)]
        results.update(sched.step())
        assert isinstance(results[tickets[1]], ValueError) and "nobody" in str(results[tickets[1]])
        assert isinstance(results[tickets[3]], Exception)
        _run_to_idle(sched, results)
        assert sched.stats["rows"] == 4
    _meets_the_yardstick(world, 0, results[tickets[0]], seen)
    _meets_the_yardstick(world, 4, results[tickets[2]], seen)


def test_server_three_threads(tts, world):
    batch = world[0]
    futures, errors = {}, []
    with _spy(tts) as (seen, threads):
        server = tts.serve(chunk=8)
        try:
            def client(c):
                try:
                    for r in (2 * c, 2 * c + 1):
                        futures[r] = server.submit(batch[r])
                except Exception as e:                   # noqa: BLE001
                    errors.append(e)
            clients = [threading.Thread(target=client, args=(c,)) for c in range(3)]
            for t in clients:
                t.start()
            for t in clients:
                t.join(WAIT)
            assert not errors and sorted(futures) == list(range(6))
            results = {r: f.result(timeout=WAIT) for r, f in futures.items()}
        finally:
            server.shutdown(timeout=WAIT)
        assert not server._thread.is_alive() and server.error is None
        assert threads == {server._thread.ident}, "only the loop thread touches the GPU"
    for r in range(6):
        _meets_the_yardstick(world, r, results[r], seen)
    assert server.scheduler.stats["rows"] == 19
    with pytest.raises(RuntimeError):
        server.submit(batch[0])


def test_run_batch_works_after_close(tts, world):
    batch, alone = world
    sched = Scheduler(tts, chunk=8)
    t = sched.submit(batch[2])
    sched.step()
    assert sched._ses is not None and not sched.idle and t == 0
    with pytest.raises(RuntimeError, match=r"rc=-3"):
        tts.run_batch([batch[0]])                        # the decoder is the open session's
    sched.close()
    assert sched._ses is None and len(sched.sessions) == 1 and sched.idle
    with pytest.raises(RuntimeError):
        sched.submit(batch[0])
    out = tts.run_batch([batch[2]])
    assert out[0][0] == alone[2][0] and np.array_equal(out[0][1], alone[2][1])
