"""GPU: "best_of" through TTS.run / TTS.run_batch / gsv.serving on the fp32 small v2 pipeline of test_run_batch_gpu.py
(max_batch 4, max_seq 256, early stop after 20 tokens, EOS reachable).

* candidate 0 is the plain draw: with best_of = 3 and a score that always picks 0, run and run_batch return the audio they
  return without the key, bit for bit, and a neighbour request without the key is unchanged;
* the default rule: last_candidates marks the highest mean log-probability among the candidates EOS ended (among all when
  every one was cut), and its means are the means of the decoder's last_logprobs;
* another candidate: a score that picks 2 gives the tokens a decode of the sentence alone with the key (seed, row + 2048) gives,
  and audio of the length those tokens give;
* serving: the request is exclusive and comes back equal to run_batch([request]).
"""
import math

import numpy as np
import pytest

from gsv.TTS_infer_pack.TTS import early_stop_num
from test_run_batch_continuous_gpu import _run_batch
from test_run_batch_gpu import _alone, _build, _segs, _voice_args
from test_run_batch_shared_gpu import BASE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tts():
    return _build("v2")


@pytest.fixture(scope="module")
def voice_kw():
    return _voice_args(0, 8, 6, "v2"), _voice_args(1, 23, 4, "v2")


REQ = dict(BASE, segments=_segs(50, [9, 5, 7]), batch_size=3, seed=3)       # one to_batch batch of three sentences
OTHER = dict(BASE, segments=_segs(51, [7, 11]), batch_size=2, seed=4)


def _same(a, b):
    return a[0] == b[0] and a[1].dtype == b[1].dtype == np.int16 and a[1].shape == b[1].shape and np.array_equal(a[1], b[1])


def test_run_candidate_0_is_the_plain_draw(tts, voice_kw):
    VA = voice_kw[0]
    plain = _alone(tts, VA, dict(REQ))
    assert tts.last_candidates == [] and np.abs(plain[1]).max() > 0
    first = _alone(tts, VA, dict(REQ, best_of=3, best_of_score=lambda c: 0))
    assert _same(plain, first), "candidate 0 must be the row a request without best_of decodes"
    rec = tts.last_candidates
    assert len(rec) == 1 and len(rec[0]) == 1 and len(rec[0][0]) == 3, "one request, one to_batch batch, three sentences"
    for sent in rec[0][0]:
        assert len(sent) == 3 and [c["chosen"] for c in sent] == [True, False, False]
        assert all(set(c) == {"n", "mean_logprob", "cut", "chosen"} for c in sent)
    assert _same(plain, _alone(tts, VA, dict(REQ, best_of=1)))
    assert tts.last_candidates == []


def test_run_batch_candidate_0_is_the_plain_draw_and_the_neighbour_is_unchanged(tts, voice_kw):
    va, vb = tts.make_voice(**voice_kw[0]), tts.make_voice(**voice_kw[1])
    plain = tts.run_batch([dict(REQ, voice=va), dict(OTHER, voice=vb)])
    assert tts.last_candidates == [[], []]
    both = tts.run_batch([dict(REQ, voice=va, best_of=3, best_of_score=lambda c: 0), dict(OTHER, voice=vb)])
    assert _same(plain[0], both[0]) and _same(plain[1], both[1])
    rec = tts.last_candidates
    assert len(rec[0][0]) == 3 and rec[1] == []
    cont = tts.run_batch([dict(REQ, voice=va, best_of=3, best_of_score=lambda c: 0), dict(OTHER, voice=vb)], continuous_ar=True)
    assert _same(plain[0], cont[0]) and _same(plain[1], cont[1])
    assert tts.last_candidates == rec, "fp32: a session decodes a row to the same bits as a launch"
    with pytest.raises(ValueError, match="best_of"):
        tts.run_batch([dict(REQ, voice=va, best_of=17)])
    with pytest.raises(ValueError, match="parallel_infer"):
        tts.run_batch([dict(REQ, voice=va, best_of=2, parallel_infer=False)])
    vfree = tts.make_voice(**_voice_args(3, 5, 0, "v2", prompt_free=True))
    with pytest.raises(ValueError, match="prompt"):
        tts.run_batch([dict(REQ, voice=vfree, best_of=2)])


def test_the_default_rule_and_its_means(tts, voice_kw):
    VA = voice_kw[0]
    out = _alone(tts, VA, dict(REQ, best_of=4))
    assert np.abs(out[1]).max() > 0
    sents = tts.last_candidates[0][0]
    lps, cuts = tts.t2s_model.last_logprobs, tts.t2s_model.last_cut
    assert len(sents) == 3 and len(lps) == 12, "three sentences, four candidates each, in (sentence, candidate) order"
    distinct = 0
    for j, sent in enumerate(sents):
        means = []
        for c, rec in enumerate(sent):
            lp = lps[4 * j + c].cpu().numpy()
            assert lp.shape == (rec["n"] + 1,) and rec["cut"] == cuts[4 * j + c] == (rec["n"] >= 20)
            want = float(lp[:rec["n"]].astype(np.float64).mean()) if rec["n"] else -math.inf
            assert rec["mean_logprob"] == want
            means.append(want)
        pool = [c for c, rec in enumerate(sent) if not rec["cut"]] or list(range(4))
        best = max(pool, key=lambda c: (means[c], -c))
        assert [rec["chosen"] for rec in sent] == [c == best for c in range(4)]
        distinct += len(set(means)) > 1
    assert distinct == 3, "the candidates of a sentence are different draws"


def test_another_candidate_is_the_row_alone_with_its_key(tts, voice_kw):
    va = tts.make_voice(**voice_kw[0])
    plain, _ = _run_batch(tts, [dict(REQ, voice=va)])
    third, preds = _run_batch(tts, [dict(REQ, voice=va, best_of=3, best_of_score=lambda c: 2)])
    assert [c["chosen"] for c in tts.last_candidates[0][0][0]] == [False, False, True]
    pl = tts._plan_request(dict(REQ, voice=va))
    assert pl["actual_seed"] == 3 and len(pl["data"]) == 1
    item, P = pl["data"][0], int(va["prompt_semantic"].numel())
    n_plain, n_third = 0, 0
    for j in range(3):
        y, idx = tts.t2s_model.infer_panel_batch_infer(
            [item["all_phones"][j]], None, [va["prompt_semantic"].view(-1)], [item["all_bert_features"][j]], top_k=REQ["top_k"],
            top_p=REQ["top_p"], temperature=REQ["temperature"], repetition_penalty=REQ["repetition_penalty"],
            early_stop_num=early_stop_num(tts.configs), rng_keys=[(3, j + 2048)])
        assert preds[0][0][j] == y[0].cpu().tolist(), f"sentence {j}: not the tokens of the key (3, {j} + 2048)"
        assert tts.last_candidates[0][0][j][2]["n"] == idx[0] == len(preds[0][0][j]) - P
        n_third += idx[0]
    _, base_preds = _run_batch(tts, [dict(REQ, voice=va)])
    n_plain = sum(len(p) - P for p in base_preds[0][0])
    per_token = 2 * math.prod(tts.vits_model.upsample_rates)
    assert third[0][1].shape[0] - plain[0][1].shape[0] == (n_third - n_plain) * per_token
    assert any(preds[0][0][j] != base_preds[0][0][j] for j in range(3)), "candidate 2 is another draw than candidate 0"


def test_a_best_of_request_is_exclusive_in_serving(tts, voice_kw):
    va, vb = tts.make_voice(**voice_kw[0]), tts.make_voice(**voice_kw[1])
    req, other = dict(REQ, voice=va, best_of=3), dict(OTHER, voice=vb)
    alone = tts.run_batch([dict(req)])[0]
    alone_rec = tts.last_candidates
    alone_other = tts.run_batch([dict(other)])[0]
    with tts.serve(chunk=8) as server:
        f_other, f_req = server.submit(dict(other)), server.submit(dict(req))
        got_other, got = f_other.result(timeout=120), f_req.result(timeout=120)
        stats = server.scheduler.stats
    assert _same(alone, got), "a best_of request through the server is run_batch([request])"
    assert got_other[0] == alone_other[0] and got_other[1].shape == alone_other[1].shape
    assert stats["exclusive"] == 1
    assert tts.last_candidates == alone_rec
