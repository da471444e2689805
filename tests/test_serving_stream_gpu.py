"""GPU: streaming (`return_fragment` / `streaming_mode`) requests inside the serving sessions, on an fp32 small v2 pipeline with
8 decoder slots (the model of test_run_batch_gpu.py, max_seq 256, early stop at 20 tokens).

The yardsticks: a streaming request's fragments are those of `list(tts.run(dict(request, return_fragment=True)))` with the
request's voice as the prompt cache -- as many, the same AR token ids per sentence, each of the same length and within 1 int16
LSB (the server's bar in test_serving_gpu.py) -- and a plain request's audio is within the same bar of run_batch([request]);
whatever else is in flight.  No streaming request is exclusive, and the whole burst is one decode session."""
import copy
import threading
from concurrent.futures import CancelledError

import numpy as np
import pytest

from gsv import synthetic as S
from gsv import wire
from gsv.serving import Scheduler, plan_online
from test_run_batch_continuous_gpu import _run_batch
from test_run_batch_gpu import DEV, _segs, _voice_args
from test_run_batch_shared_gpu import BASE, _lsb
from test_serving_gpu import _spy

pytestmark = pytest.mark.gpu

WAIT = 120.0
STREAMS = (0, 2, 4)


@pytest.fixture(scope="module")
def tts():
    from gsv.TTS_infer_pack.TTS import TTS
    tcfg = S.small_t2s_config(n_layer=2, dim=128, head=4, vocab=1025, phoneme_vocab=732)
    tcfg["data"]["max_sec"] = 0.4                           # early_stop_num = 20 tokens
    tsd = S.make_t2s_state_dict(tcfg, seed=11, suppress_eos=False)
    vcfg = copy.deepcopy(S.small_vits_config())
    vsd = S.make_vits_state_dict(vcfg, seed=12)
    tts = TTS({"device": DEV, "is_half": False, "version": "v2", "max_batch": 8, "max_seq": 256})
    tts.init_t2s_weights(state={"weight": tsd, "config": tcfg})
    tts.init_vits_weights(state={"weight": vsd, "config": vcfg})
    return tts


def _run_stream(tts, voice_kw, req):
    """run()'s fragments of the request and the AR tokens [bi][j] it decoded (prompt included)"""
    tts.set_prompt_cache(**voice_kw)
    toks, inner = [], tts._synthesize_batch

    def spy(item, pred, pred_list, *a, **k):
        toks.append([p.cpu().tolist() for p in pred_list])
        return inner(item, pred, pred_list, *a, **k)
    tts._synthesize_batch = spy
    try:
        frags = list(tts.run(dict(req, return_fragment=True)))
    finally:
        del tts._synthesize_batch
    return frags, toks


@pytest.fixture(scope="module")
def world(tts):
    """six requests, three of them streaming (0: folds of 2 + 1 sentences; 2: 2 + 2 + 1; 4: one sentence at speed 1.25, which
    no shared pass takes), each with its yardstick: run()'s fragments and tokens / run_batch([request])'s audio and tokens"""
    va, vb, vc = _voice_args(0, 8, 6, "v2"), _voice_args(1, 23, 4, "v2"), _voice_args(2, 5, 7, "v2")
    other = dict(BASE, top_k=12, top_p=0.9, temperature=0.8, repetition_penalty=1.2)
    reqs = [(va, dict(BASE, segments=_segs(50, [9, 5, 7]), batch_size=2, seed=3, return_fragment=True)),
            (vb, dict(other, segments=_segs(51, [7, 12, 6]), batch_size=2, seed=4)),
            (vc, dict(other, segments=_segs(52, [11, 6, 8, 5, 10]), batch_size=2, seed=5, streaming_mode=True)),
            (va, dict(BASE, segments=_segs(53, [6, 9]), seed=6)),
            (vb, dict(BASE, segments=_segs(54, [10]), seed=7, speed_factor=1.25, return_fragment=True)),
            (vc, dict(BASE, segments=_segs(55, [8, 7, 13]), batch_size=2, seed=8))]
    alone = []
    for r, (kw, req) in enumerate(reqs):
        if r in STREAMS:
            plain = {k: v for k, v in req.items() if k not in ("return_fragment", "streaming_mode")}
            alone.append(_run_stream(tts, kw, plain))
    voices = {}
    for kw, _ in reqs:
        voices.setdefault(id(kw), tts.make_voice(**kw))
    batch = [dict(req, voice=voices[id(kw)]) for kw, req in reqs]
    full, s = [], iter(alone)
    for r, req in enumerate(batch):
        if r in STREAMS:
            full.append(next(s))
        else:
            out, preds = _run_batch(tts, [req])
            full.append((out[0], preds[0]))
    assert [len(full[r][0]) for r in STREAMS] == [2, 3, 1] and all(np.abs(f[1]).max() > 0 for r in STREAMS for f in full[r][0])
    return batch, full


def _tokens(pl):
    return [[p.cpu().tolist() for p in pred] for pred in pl["preds"]]


def _stream_meets_the_yardstick(world, r, result, tokens):
    frags, toks = world[1][r]
    assert not isinstance(result, BaseException), f"request {r} raised {result!r}"
    assert isinstance(result, list) and len(result) == len(frags), f"request {r}: {len(result)} fragments, run() yields {len(frags)}"
    assert tokens == toks, f"request {r}: a sentence decodes other tokens than in run()"
    for bi, ((sr, a), (sr0, a0)) in enumerate(zip(result, frags)):
        assert sr == sr0 and a.dtype == np.int16 and a.shape == a0.shape, f"request {r} fragment {bi}: {a.shape} vs {a0.shape}"
        assert _lsb(a, a0) <= 1, f"request {r} fragment {bi}: {_lsb(a, a0)} LSB from run()'s fragment"


def _plain_meets_the_yardstick(world, r, result, seen):
    (sr, audio), tokens = world[1][r]
    assert not isinstance(result, BaseException), f"request {r} raised {result!r}"
    assert seen[world[0][r]["seed"]][0] == tokens
    assert result[0] == sr and result[1].dtype == np.int16 and result[1].shape == audio.shape
    assert _lsb(result[1], audio) <= 1, f"request {r}: {_lsb(result[1], audio)} LSB from run_batch([request])"


def _drive(sched, batch, schedule, plans, results, frag_steps, limit=400):
    """schedule[s]: the requests submitted in front of step s; then steps until idle.  plans: ticket -> the plan of a streaming
    request (kept so that its tokens can be read when it is done); frag_steps: ticket -> the step of each of its fragments"""
    ticket_of, n = {}, 0
    todo = list(schedule)
    while todo or not sched.idle:
        for r in (todo.pop(0) if todo else []):
            ticket_of[r] = sched.submit(batch[r])
        results.update(sched.step())
        for t, pl in sched._requests.items():
            if isinstance(pl, dict) and "stream" in pl:
                plans.setdefault(t, pl)
        for t, bi, (sr, a) in sched.take_fragments():
            assert bi == len(frag_steps.setdefault(t, [])), "fragments come in fold order"
            frag_steps[t].append(sched.stats["steps"] - 1)
        assert sched.take_fragments() == []
        n += 1
        assert n <= limit, "the scheduler does not come to rest"
    return ticket_of


@pytest.mark.parametrize("chunk", [1, 8])
def test_staggered_streaming_and_plain_requests(tts, world, chunk):
    batch = world[0]
    results, plans, frag_steps = {}, {}, {}
    with _spy(tts) as (seen, _), Scheduler(tts, slots=8, chunk=chunk) as sched:
        ticket_of = _drive(sched, batch, [[0, 1], [2], [3], [4, 5]], plans, results, frag_steps)
        stats, sessions = sched.stats, sched.sessions
        assert sched._ses is None
    assert [ticket_of[r] for r in range(6)] == list(range(6)) and sorted(results) == list(range(6))
    for r in range(6):
        if r in STREAMS:
            _stream_meets_the_yardstick(world, r, results[r], _tokens(plans[r]))
            assert [f[1].tolist() for f in results[r]] == [f[1].tolist() for f in plans[r]["stream"]]
            assert len(frag_steps[r]) == len(results[r]) and frag_steps[r][-1] == stats["tickets"][r][2]
        else:
            _plain_meets_the_yardstick(world, r, results[r], seen)
    # nobody was a barrier: one session for the burst, and it was never drained
    assert stats["exclusive"] == 0 and stats["sessions"] == 1 == len(sessions)
    assert not any(e[0] == "exclusive" for e in stats["events"]) and [e for e in stats["events"] if e[0] == "close"] == [("close",)]
    # the recorded events are plan_online's, fed with the arrivals, the measured lengths and the streaming requests' folds
    idxs = {r: [[int(i) for i in idx] for idx in plans[r]["idxs"]] if r in STREAMS else seen[batch[r]["seed"]][1] for r in range(6)}
    lengths = [n for r in range(6) for idx in idxs[r] for n in idx]
    plan = plan_online([stats["tickets"][t][0] for t in range(6)], [len(batch[r]["segments"]) for r in range(6)], lengths, slots=8,
                       chunk=chunk, streaming={r: [len(idx) for idx in idxs[r]] for r in STREAMS})
    assert stats["events"] == plan
    assert sum(e[0] == "fragment" for e in plan) == 6
    if chunk == 1:
        # a multi-sentence streaming request hands out its first fragment in an earlier step than its last
        assert any(frag_steps[r][0] < frag_steps[r][-1] for r in (0, 2)), frag_steps


def test_cancel_after_the_first_fragment(tts, world):
    batch = world[0]
    results, plans, frags = {}, {}, {}
    with _spy(tts) as (seen, _), Scheduler(tts, slots=8, chunk=1) as sched:
        ticket_of = {r: sched.submit(batch[r]) for r in (1, 3, 2, 0, 5)}
        victim = None
        for _ in range(200):
            results.update(sched.step())
            for t, bi, f in sched.take_fragments():
                frags.setdefault(t, []).append(f)
            mid = [t for t in frags if t in sched._pol.missing]         # a fragment is out and sentences are still decoding
            if mid:
                victim = mid[0]
                break
        assert victim is not None, "no streaming request was caught between its first fragment and its last sentence"
        held = [s for s, o in enumerate(sched._pol.owner) if o is not None and o[0] == victim]
        assert sched.cancel(victim) and not sched.cancel(victim)
        assert all(o is None or o[0] != victim for o in sched._pol.owner) and victim not in sched._pol.stream
        assert sched._ses.state()[1].tolist() == [int(o is not None) for o in sched._pol.owner], "the live rows are released"
        if held:
            assert sched.stats["events"][-1] == ("release", held)
        n = 0
        while not sched.idle:
            results.update(sched.step())
            for t, pl in sched._requests.items():
                if isinstance(pl, dict) and "stream" in pl:
                    plans.setdefault(t, pl)
            assert not any(t == victim for t, _, _ in sched.take_fragments()), "a cancelled stream emits nothing more"
            n += 1
            assert n <= 400
    assert isinstance(results[victim], CancelledError) and len(frags[victim]) >= 1
    for r, t in ticket_of.items():
        if t == victim:
            continue
        if r in STREAMS:
            if t in plans:                          # (a stream that ended before the cancel has no plan left to read)
                _stream_meets_the_yardstick(world, r, results[t], _tokens(plans[t]))
            else:
                frs = world[1][r][0]
                assert len(results[t]) == len(frs) and all(_lsb(a[1], b[1]) <= 1 for a, b in zip(results[t], frs))
        else:
            _plain_meets_the_yardstick(world, r, results[t], seen)


def test_three_threads_submit_stream_and_the_wire_seam(tts, world):
    batch = world[0]
    got, errors = {}, []
    server = tts.serve(slots=8, chunk=4)

    class Tap:
        """the server as tts_handle sees it, remembering the streams it opened"""
        streams = []

        def submit(self, req):
            return server.submit(req)

        def submit_stream(self, req):
            self.streams.append(server.submit_stream(req))
            return self.streams[-1]
    try:
        def client(c):
            try:
                r, p = STREAMS[c], (1, 3, 5)[c]
                stream, fut = server.submit_stream(batch[r]), server.submit(batch[p])
                got[r] = (list(stream), stream.future.result(timeout=WAIT))
                got[p] = fut.result(timeout=WAIT)
            except Exception as e:                   # noqa: BLE001
                errors.append(e)
        clients = [threading.Thread(target=client, args=(c,)) for c in range(3)]
        for t in clients:
            t.start()
        for t in clients:
            t.join(WAIT)
        assert not errors and sorted(got) == list(range(6))
        for r in STREAMS:
            frs = world[1][r][0]
            seen_frags, final = got[r]
            assert len(seen_frags) == len(final) == len(frs) and all(a[1] is b[1] for a, b in zip(seen_frags, final))
            assert all(a[0] == b[0] and a[1].shape == b[1].shape and _lsb(a[1], b[1]) <= 1 for a, b in zip(final, frs))
        for r in (1, 3, 5):
            (sr, audio), _ = world[1][r]
            assert got[r][0] == sr and got[r][1].shape == audio.shape and _lsb(got[r][1], audio) <= 1
        # a stream that is cancelled ends with CancelledError
        stream = server.submit_stream(batch[2])
        stream.cancel()
        with pytest.raises(CancelledError):
            list(stream)
        # the wire layer frames the fragments of the stream it opened, as streaming_generator frames them
        tap = Tap()
        for media in ("raw", "wav"):
            code, mt, payload = wire.tts_handle(tts, dict(batch[0], streaming_mode=True, media_type=media), server=tap)
            assert code == 200 and mt == f"audio/{media}"
            chunks = list(payload)
            final = tap.streams[-1].future.result(timeout=WAIT)
            assert len(final) == 2 and chunks == list(wire.streaming_generator(iter(final), media))
        assert server.scheduler.stats["exclusive"] == 0
    finally:
        server.shutdown(timeout=WAIT)
    assert not server._thread.is_alive() and server.error is None
