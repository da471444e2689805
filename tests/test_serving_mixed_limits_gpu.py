"""GPU: Scheduler(mixed_limits=True) -- prompt-free, parallel_infer=False, best_of and arena-short requests as citizens of the
open decode session.  fp32 small v2 pipeline (EOS-prone head, max_batch 8, max_seq 256), 6 slots, eight requests: two plain,
one prompt-free, one naive, one streaming naive, one with a sentence that leaves 15 of the 21 steps, one best_of=3 and one
streaming best_of=2.

The yardstick is the server's: a request's result is what run_batch([request]) gives for it alone (run() for a streaming one)
-- the same tokens per sentence (the same chosen candidate), audio within 1 int16 LSB.  For the run, at chunk 2 with arrivals
one step apart and at chunk 5 with arrivals three steps apart: no exclusive request, ONE session, and the events plan_online
gives for the arrivals and the measured row lengths with exclusive=().

The input is checked on the CPU, with the oracle, before any device work.  EOS shows: at least two rows end by EOS before
step 11 under horizon 1 and run past step 10 under horizon 11.  And the requests overlap at 15 decode steps between arrivals:
every request that another follows holds a greedy row of 16 tokens or more (four advances of 5), and the two requests that
sample (best_of) come last, behind a plain request of 8 such rows on the 6 slots, whose last two rows decode until both have
arrived.  One case on the fp32 small v3 pipeline with continuous_cfm=True: a plain and a best_of=2 request, 0 int16 LSB from
run_batch([request], shared_cfm=True)."""
from concurrent.futures import CancelledError

import numpy as np
import pytest

from gsv.serving import Scheduler, plan_online
from test_run_batch_continuous_gpu import _run_batch
from test_run_batch_gpu import _segs, _voice_args
from test_run_batch_mixed_limits_gpu import build, t2s_weights
from test_run_batch_shared_gpu import BASE, _lsb
from test_serving_gpu import _run_to_idle, _spy

pytestmark = pytest.mark.gpu
SLOTS = 6


@pytest.fixture(scope="module")
def tts():
    return build(max_batch=8)


LENS = [6, 9, 7, 8, 5, 10, 6, 7]          # sentence k of a request has LENS[k] phones (the 225-phone sentence apart)
VOICES = [(0, 8, 6), (1, 23, 4)]          # (voice number, prompt tokens, prompt phones)
GREEDY = dict(BASE, top_k=1)              # the oracle can say how long a greedy row runs
# (voice or None: prompt-free, segment seed, sentences, request keys, EOS horizon run_batch gives its rows)
REQUESTS = [
    (0, 60, 3, dict(GREEDY, batch_size=2, seed=11), 1),                                            # 0 plain
    (None, 66, 2, dict(GREEDY, batch_size=2, seed=12), 11),                                        # 1 prompt-free
    (1, 68, 2, dict(GREEDY, batch_size=2, seed=13, parallel_infer=False), 11),                     # 2 naive
    (1, 63, 2, dict(GREEDY, batch_size=1, seed=15, parallel_infer=False, return_fragment=True), 11),   # 3 streaming naive
    (0, 60, 1, dict(GREEDY, batch_size=1, seed=16), 1),                                            # 4 arena-short: + 225 phones
    (0, 62, 8, dict(GREEDY, batch_size=8, seed=17), 1),                                            # 5 plain, 8 rows on 6 slots
    (0, 63, 2, dict(BASE, batch_size=2, seed=14, best_of=3, top_k=15), 1),                         # 6 best_of
    (0, 67, 2, dict(BASE, batch_size=1, seed=18, best_of=2, top_k=15, return_fragment=True), 1),   # 7 streaming best_of
]
ROWS = [3, 2, 2, 2, 2, 8, 6, 4]
STREAMS = (3, 7)
BEST_OF = 6


def _segments(r):
    seed, n = REQUESTS[r][1], REQUESTS[r][2]
    segs = _segs(seed, LENS[:n])
    return segs + _segs(65, [225]) if r == 4 else segs


def _oracle_input_check():
    """the docstring's two conditions, from the CPU oracle alone; a failure is a bad input, not a parity failure"""
    import torch
    from gsv import synthetic as S
    from oracle.t2s_oracle import T2SOracle
    tcfg, tsd = t2s_weights()
    orc = T2SOracle(tsd, tcfg)
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, repetition_penalty=BASE["repetition_penalty"], early_stop_num=20, max_steps=21)
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        shows = 0
        for r, (voice, seed, n, req, horizon) in enumerate(REQUESTS[:6]):
            vi, P, n_ph = (3, 5, 0) if voice is None else VOICES[voice]
            sem = torch.from_numpy(S.hash_ints(f"rb_sem{vi}", P, 1024, 7)).long()
            head = S.hash_ints(f"rb_ph{vi}", n_ph, 732, 7).tolist() if n_ph else []
            ends = []
            for k in range(n):
                x = torch.tensor(head + S.hash_ints(f"rb_seg{seed}_{k}", LENS[k], 732, 9).tolist())
                prompt = (sem if n_ph else sem[:0]).unsqueeze(0)
                h1, h11 = (orc.infer_panel_batch_infer([x], None, prompt, [torch.zeros(1024, x.numel())], eos_mask_steps=e, **kw)[1][0]
                           for e in (1, 11))
                shows += h1 < 11 and h11 > 10
                ends.append(h1 if horizon == 1 else h11)
            assert max(ends) >= 16 and (r != 5 or min(ends) >= 16), f"bad input: request {r} decodes {ends} tokens (oracle)"
        assert shows >= 2, "bad input: the EOS horizon does not show"
    finally:
        torch.set_num_threads(threads)


@pytest.fixture(scope="module")
def world(tts):
    """the eight requests, and what run_batch([request]) (run() for a streaming one) returns for each alone"""
    _oracle_input_check()
    vkw = [_voice_args(i, P, n_ph, "v2") for i, P, n_ph in VOICES]
    v = [tts.make_voice(**kw) for kw in vkw]
    vfree = tts.make_voice(**_voice_args(3, 5, 0, "v2", prompt_free=True))
    batch = [dict(req, segments=_segments(r), voice=vfree if voice is None else v[voice])
             for r, (voice, _, _, req, _) in enumerate(REQUESTS)]
    assert [len(b["segments"]) * b.get("best_of", 1) for b in batch] == ROWS
    alone = []
    for r, req in enumerate(batch):
        if req.get("return_fragment"):
            tts.set_prompt_cache(**vkw[REQUESTS[r][0]])    # run() reads the prompt cache, not the request's voice
            alone.append(list(tts.run({k: x for k, x in req.items() if k != "voice"})))
            continue
        out, preds = _run_batch(tts, [dict(req)])
        alone.append((out[0][0], out[0][1], preds[0], list(tts.last_candidates[0])))
        assert np.abs(out[0][1]).max() > 0
    return batch, alone


def _check(world, r, result, seen, cands):
    batch, alone = world
    assert not isinstance(result, BaseException), f"request {r} raised {result!r}"
    if batch[r].get("return_fragment"):
        assert len(result) == len(alone[r])
        for (sr_a, a), (sr_b, b) in zip(alone[r], result):
            assert sr_a == sr_b and a.shape == b.shape and _lsb(a, b) <= 1
        return
    sr, audio, tokens, chosen = alone[r]
    assert seen[batch[r]["seed"]][0] == tokens, f"request {r}: a sentence decodes other tokens than in run_batch([request])"
    assert result[0] == sr and result[1].dtype == np.int16 and result[1].shape == audio.shape
    assert _lsb(result[1], audio) <= 1, f"request {r}: {_lsb(result[1], audio)} LSB from run_batch([request])"
    assert cands.get(batch[r]["seed"], []) == chosen, f"request {r}: other candidates than run_batch([request])"


def _watch(sched, tts, lengths, folds, cands):
    """records every row's length by (ticket, row), every streaming request's rows per fold, every finished plan's candidates"""
    advance, arrive, finish = sched._advance, sched._pol.arrive, tts._finish_request

    def adv(chunk):
        ses, where = sched._ses, dict(sched._where)
        inner = ses.advance

        def spy(steps):
            out = inner(steps)
            lengths.update({where[st]: n for st, _, n in out})
            return out
        ses.advance = spy
        try:
            return advance(chunk)
        finally:
            del ses.advance

    def arr(req, rows, exclusive, step, f=None):
        if f:
            folds[req] = list(f)
        return arrive(req, rows, exclusive, step, f)

    def fin(pl, sr):
        cands[pl["actual_seed"]] = pl.get("candidates", [])
        return finish(pl, sr)
    sched._advance, sched._pol.arrive, tts._finish_request = adv, arr, fin
    return finish


@pytest.mark.parametrize("chunk,gap", [(2, 1), (5, 3)])
def test_eight_requests_one_session_no_exclusive(tts, world, chunk, gap):
    batch = world[0]
    N = len(batch)
    results, ticket_of, lengths, folds, cands = {}, {}, {}, {}, {}
    with _spy(tts) as (seen, _), Scheduler(tts, slots=SLOTS, chunk=chunk, mixed_limits=True) as sched:
        restore = _watch(sched, tts, lengths, folds, cands)
        try:
            for r in range(N):
                ticket_of[r] = sched.submit(dict(batch[r]))
                for _ in range(gap):
                    results.update(sched.step())
            _run_to_idle(sched, results, limit=200)
        finally:
            tts._finish_request = restore
        stats, sessions = sched.stats, sched.sessions
    for r, t in ticket_of.items():
        _check(world, r, results[t], seen, cands)
    flat = [lengths[(t, k)] for t in range(N) for k in range(ROWS[t])]
    print(f"[serving mixed limits] chunk {chunk}: row lengths {flat}")
    assert stats["exclusive"] == 0 and stats["sessions"] == 1 == len(sessions) and sessions[0].slots == SLOTS
    assert stats["rows"] == sum(ROWS) == len(sessions[0].history)
    assert [ticket_of[r] for r in range(N)] == list(range(N))
    assert folds == {3: [1, 1], 7: [2, 2]}, "a streaming best_of fold counts its candidate rows"
    plan = plan_online([stats["tickets"][t][0] for t in range(N)], ROWS, flat, slots=SLOTS, chunk=chunk, exclusive=(),
                       streaming={t: folds[t] for t in STREAMS})
    assert stats["events"] == plan
    assert len(set(flat)) > 2


def test_cancelling_a_best_of_request_releases_all_its_candidate_rows(tts, world):
    batch = world[0]
    results = {}
    with _spy(tts) as (seen, _), Scheduler(tts, slots=SLOTS, chunk=1, mixed_limits=True) as sched:
        cands = {}
        restore = _watch(sched, tts, {}, {}, cands)
        try:
            t3 = sched.submit(dict(batch[BEST_OF]))
            results.update(sched.step())
            assert sched.stats["events"][0] == ("admit", [(t3, k, k) for k in range(6)])
            live = sched._ses.state()[1].tolist()
            assert sum(live) >= 1, "candidate rows must still be decoding when the request is cancelled"
            assert sched.cancel(t3)
            assert sched.stats["released"] == sum(live) and sched._ses.state()[1].tolist() == [0] * SLOTS
            assert not sched._cands
            t0 = sched.submit(dict(batch[0]))
            _run_to_idle(sched, results)
        finally:
            tts._finish_request = restore
    assert isinstance(results[t3], CancelledError)
    _check(world, 0, results[t0], seen, cands)


def test_v3_best_of_through_both_sessions():
    from test_pipeline_v3_gpu import _build as build_v3
    from test_run_batch_cfm_gpu import BASE as BASE3, _voice
    tts, *_ = build_v3("v3")
    va, vb = _voice(0, 8, 6, 14, "v3"), _voice(1, 14, 4, 31, "v3")
    batch = [dict(BASE3, segments=_segs(20, [9, 5]), batch_size=2, seed=3, voice=tts.make_voice(**va)),
             dict(BASE3, segments=_segs(22, [11, 6]), batch_size=2, seed=5, voice=tts.make_voice(**vb), best_of=2)]
    alone = []
    for req in batch:
        out, preds = _run_batch(tts, [dict(req)], shared_cfm=True)
        alone.append((out[0][0], out[0][1], preds[0], list(tts.last_candidates[0])))
    results, cands = {}, {}
    with _spy(tts) as (seen, _), Scheduler(tts, chunk=8, continuous_cfm=True, mixed_limits=True) as sched:
        restore = _watch(sched, tts, {}, {}, cands)
        try:
            tickets = []
            for req in batch:
                tickets.append(sched.submit(dict(req)))
                results.update(sched.step())
            _run_to_idle(sched, results)
        finally:
            tts._finish_request = restore
        stats = sched.stats
    assert stats["exclusive"] == 0 and stats["rows"] == 2 + 4
    for r, t in enumerate(tickets):
        sr, audio, tokens, chosen = alone[r]
        assert not isinstance(results[t], BaseException), results[t]
        assert seen[batch[r]["seed"]][0] == tokens and cands[batch[r]["seed"]] == chosen
        assert results[t][0] == sr and results[t][1].shape == audio.shape
        print(f"[serving mixed limits] v3 request {r}: {_lsb(results[t][1], audio)} LSB from run_batch([request], shared_cfm=True)")
        assert _lsb(results[t][1], audio) == 0
