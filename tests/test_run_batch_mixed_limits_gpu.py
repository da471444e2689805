"""GPU: run_batch(mixed_sampling=True, mixed_limits=True) on the fp32 small v2 pipeline -- a plain, a parallel_infer=False, a
prompt-free and a best_of=3 request, two sentences each, share ONE AR launch where run_batch needs four, and every request
gets the tokens (and the candidate) it gets without the keywords, audio within 1 int16 LSB.

The T2S weights have their EOS row scaled by -1.4: random weights never emit EOS, and without one the EOS horizon of the naive
and prompt-free rows (11 steps against 1) would not show.  With it the CPU oracle ends about half the greedy rows of these
voices by EOS (after 5 .. 15 tokens under horizon 1, 12 .. 20 under horizon 11) and lets the others run into the early stop."""
import copy

import numpy as np
import pytest

from test_run_batch_continuous_gpu import _run_batch
from test_run_batch_gpu import DEV, _segs, _voice_args
from test_run_batch_shared_gpu import BASE, _lsb

pytestmark = pytest.mark.gpu
EOS_GAIN = -1.4


def t2s_weights():
    """config and EOS-prone state dict of the pipeline's T2S model (no GPU needed: the CPU oracle takes them too)"""
    from gsv import synthetic as S
    tcfg = S.small_t2s_config(n_layer=2, dim=128, head=4, vocab=1025, phoneme_vocab=732)
    tcfg["data"]["max_sec"] = 0.4                           # early_stop_num = 20 tokens
    tsd = S.make_t2s_state_dict(tcfg, seed=11, suppress_eos=False)
    tsd["ar_predict_layer.weight"][1024] *= EOS_GAIN
    return tcfg, tsd


def build(version="v2", max_batch=16, max_seq=256):
    """test_run_batch_gpu._build with room for more rows and an EOS-prone head"""
    from gsv import synthetic as S
    from gsv.TTS_infer_pack.TTS import TTS
    tcfg, tsd = t2s_weights()
    vcfg = copy.deepcopy(S.small_vits_config())
    vsd = S.make_vits_state_dict(vcfg, seed=12)
    tts = TTS({"device": DEV, "is_half": False, "version": version, "max_batch": max_batch, "max_seq": max_seq})
    tts.init_t2s_weights(state={"weight": tsd, "config": tcfg})
    tts.init_vits_weights(state={"weight": vsd, "config": vcfg})
    return tts


def four_kinds(tts):
    """plain, naive, prompt-free, best_of=3 (with another top_k: a launch group of its own without the keywords)"""
    voices = [tts.make_voice(**_voice_args(i, P, n_ph, "v2")) for i, (P, n_ph) in enumerate([(8, 6), (23, 4)])]
    vfree = tts.make_voice(**_voice_args(3, 5, 0, "v2", prompt_free=True))
    return [
        dict(BASE, segments=_segs(50, [9, 6]), batch_size=2, seed=3, voice=voices[0]),
        dict(BASE, segments=_segs(51, [7, 8]), batch_size=2, seed=4, voice=voices[1], parallel_infer=False),
        dict(BASE, segments=_segs(52, [6, 10]), batch_size=2, seed=5, voice=vfree),
        dict(BASE, segments=_segs(53, [5, 8]), batch_size=2, seed=6, voice=voices[0], best_of=3, top_k=15),
    ]


def test_four_kinds_share_one_launch_and_keep_their_tokens():
    tts = build()
    reqs = four_kinds(tts)
    calls = []
    run = tts.t2s_model._run

    def counted(*a, **kw):
        calls.append(kw.get("row_limits"))
        return run(*a, **kw)
    tts.t2s_model._run = counted
    plain, tok_plain = _run_batch(tts, [dict(r) for r in reqs])
    cand_plain = copy.deepcopy(tts.last_candidates)
    assert len(calls) == 4 and all(c is None for c in calls)
    calls.clear()
    mixed, tok_mixed = _run_batch(tts, [dict(r) for r in reqs], mixed_sampling=True, mixed_limits=True)
    assert len(calls) == 1 and len(calls[0]) == 2 + 2 + 2 + 6
    assert sorted(set(calls[0])) == [(1, 20, 21), (11, 20, 21)]
    lens = [[len(t) for pred in req for t in pred] for req in tok_plain]
    print(f"[mixed limits] tokens per sentence (prompt included) {lens}; candidates {tts.last_candidates[3]}")
    assert tok_mixed == tok_plain, "mixed_limits changed a sentence's tokens"
    assert len({n for req in lens for n in req}) > 2, "the rows must end at different steps: EOS has to show"
    assert tts.last_candidates == cand_plain and cand_plain[3], "the best_of request must keep its candidates and its choice"
    for r, ((sr_a, a), (sr_b, b)) in enumerate(zip(plain, mixed)):
        assert sr_a == sr_b and a.dtype == b.dtype == np.int16 and a.shape == b.shape
        assert _lsb(a, b) <= 1, f"request {r}: {_lsb(a, b)} LSB from run_batch without the keywords"
        assert np.abs(a).max() > 0
    # a launch whose rows agree on the limits takes the scalar path
    calls.clear()
    _run_batch(tts, [dict(reqs[0]), dict(reqs[3])], mixed_sampling=True, mixed_limits=True)
    assert calls == [None]
