"""GPU: TTS.run_batch -- requests with different reference voices through shared AR decodes -- returns, per request, what
TTS.run returns for that request alone (int16 arrays equal), and leaves the prompt cache alone."""
import copy

import numpy as np
import pytest
import torch

from gsv import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _build(version):
    from gsv.TTS_infer_pack.TTS import TTS
    tcfg = S.small_t2s_config(n_layer=2, dim=128, head=4, vocab=1025, phoneme_vocab=732)
    tcfg["data"]["max_sec"] = 0.4                           # early_stop_num = 20 tokens
    tsd = S.make_t2s_state_dict(tcfg, seed=11, suppress_eos=False)
    vcfg = copy.deepcopy(S.small_vits_config())
    if version == "v2Pro":
        vcfg["model"]["version"], vcfg["model"]["gin_channels"] = "v2Pro", 1024
    vsd = S.make_vits_state_dict(vcfg, seed=12)
    tts = TTS({"device": DEV, "is_half": False, "version": version, "max_batch": 4, "max_seq": 256})
    tts.init_t2s_weights(state={"weight": tsd, "config": tcfg})
    tts.init_vits_weights(state={"weight": vsd, "config": vcfg})
    return tts


def _voice_args(i, P, n_ph, version, prompt_free=False, frames=30):
    """components of voice i as set_prompt_cache takes them"""
    kw = dict(prompt_semantic=torch.from_numpy(S.hash_ints(f"rb_sem{i}", P, 1024, 7)),
              refer_spec=[S.make_refer_spec(frames=frames + 3 * i, seed=40 + i).to(DEV)])
    if not prompt_free:
        kw.update(phones=S.hash_ints(f"rb_ph{i}", n_ph, 732, 7).tolist(), bert_features=torch.zeros(1024, n_ph),
                  norm_text="x" * n_ph)
    if version == "v2Pro":
        kw["sv_emb"] = [S.hash_symmetric(f"rb_sv{i}", (1, 20480), 1.0, 7).to(DEV)]
    return kw


def _segs(seed, lens):
    return [{"phones": S.hash_ints(f"rb_seg{seed}_{k}", n, 732, 9).tolist(), "bert_features": torch.zeros(1024, n),
             "norm_text": "y" * (3 + (k * 5 + seed) % 7)} for k, n in enumerate(lens)]


def _alone(tts, voice_kw, req):
    tts.set_prompt_cache(**voice_kw)
    out = list(tts.run(req))
    assert len(out) == 1
    return out[0]


@pytest.mark.parametrize("version", ["v2", "v2Pro"])
def test_run_batch_equals_run_per_request(version):
    tts = _build(version)
    va = _voice_args(0, 8, 6, version)
    vb = _voice_args(1, 23, 4, version)
    vc = _voice_args(2, 5, 7, version)
    vfree = _voice_args(3, 5, 0, version, prompt_free=True)
    base = dict(top_k=5, top_p=1.0, temperature=1.0, repetition_penalty=1.35, fragment_interval=0.01)
    reqs = [
        (va, dict(base, segments=_segs(0, [9, 5]), seed=3)),
        (va, dict(base, segments=_segs(1, [7]), seed=4)),                               # shares voice a
        (vb, dict(base, segments=_segs(2, [11, 6, 8]), batch_size=2, seed=5)),          # two batches of to_batch
        (vfree, dict(base, segments=_segs(3, [6, 9]), batch_size=2, seed=6)),           # prompt-free: the naive loop
        (vc, dict(base, segments=_segs(4, [10]), speed_factor=1.25, seed=7)),           # per-fragment decodes
    ]
    alone = [_alone(tts, kw, dict(req)) for kw, req in reqs]
    voices = {}
    for kw, _ in reqs:
        voices.setdefault(id(kw), tts.make_voice(**kw))
    tts.set_prompt_cache(**vb)
    cache = dict(tts.prompt_cache)
    out = tts.run_batch([dict(req, voice=voices[id(kw)]) for kw, req in reqs])
    assert tts.prompt_cache.keys() == cache.keys() and all(tts.prompt_cache[k] is cache[k] for k in cache), \
        "run_batch changed the prompt cache"
    assert len(out) == len(reqs)
    for r, ((sr_a, a), (sr_b, b)) in enumerate(zip(alone, out)):
        assert sr_a == sr_b == 32000
        assert a.dtype == b.dtype == np.int16 and a.shape == b.shape, f"request {r}: {a.shape} vs {b.shape}"
        assert np.array_equal(a, b), f"request {r}: run_batch differs from run() alone"
        assert np.abs(a).max() > 0
    # the same text in two voices must sound different (a stale style vector would make them equal)
    seg = _segs(9, [8])
    two = tts.run_batch([dict(base, segments=seg, seed=1, voice=voices[id(va)]),
                         dict(base, segments=seg, seed=1, voice=voices[id(vb)])])
    assert not np.array_equal(two[0][1], two[1][1])
    # run() after run_batch still uses the prompt cache's voice
    assert np.array_equal(list(tts.run(dict(reqs[2][1])))[0][1], alone[2][1])
    with pytest.raises(ValueError):
        tts.run_batch([dict(reqs[0][1], return_fragment=True, voice=voices[id(va)])])


def test_run_batch_v3_equals_run_per_request():
    from test_pipeline_v3_gpu import _build as build_v3
    tts, *_ = build_v3("v3")
    vs = []
    for i, (P, n_ph, Tm) in enumerate([(8, 6, 26), (14, 4, 31)]):
        kw = _voice_args(10 + i, P, n_ph, "v3")
        kw["ref_mel"] = S.hash_symmetric(f"rb_mel{i}", (1, 100, Tm), 5.0, 3) - 5.0
        vs.append(kw)
    base = dict(top_k=5, sample_steps=2, fragment_interval=0.01)
    reqs = [(vs[0], dict(base, segments=_segs(20, [9, 6]), batch_size=2, seed=3)),
            (vs[1], dict(base, segments=_segs(21, [7]), seed=4)),
            (vs[1], dict(base, segments=_segs(22, [8, 5]), batch_size=2, seed=5, parallel_infer=False))]
    alone = [_alone(tts, kw, dict(req)) for kw, req in reqs]
    voices = [tts.make_voice(**kw) for kw, _ in reqs]
    out = tts.run_batch([dict(req, voice=v) for (_, req), v in zip(reqs, voices)])
    for r, ((sr_a, a), (sr_b, b)) in enumerate(zip(alone, out)):
        assert sr_a == sr_b == 24000
        assert a.shape == b.shape and np.array_equal(a, b), f"request {r}: run_batch differs from run() alone"
