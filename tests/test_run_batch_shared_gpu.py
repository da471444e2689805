"""GPU: TTS.run_batch(shared_sovits=True) -- the waveform stage of all shareable folds in one segmented SoVITS pass --
against TTS.run per request (fp32: at most 1 LSB of the int16 output) and against run_batch without it (fp16, v3)."""
import copy

import numpy as np
import pytest
import torch

from gsv import synthetic as S
from test_run_batch_gpu import DEV, _alone, _build, _segs, _voice_args

pytestmark = pytest.mark.gpu

BASE = dict(top_k=5, top_p=1.0, temperature=1.0, repetition_penalty=1.35, fragment_interval=0.01)


def _mix(version):
    """the five requests of test_run_batch_equals_run_per_request plus one whose voice has two reference spectrograms
    (what aux_ref_audio_paths stores)"""
    va = _voice_args(0, 8, 6, version)
    vb = _voice_args(1, 23, 4, version)
    vc = _voice_args(2, 5, 7, version)
    vfree = _voice_args(3, 5, 0, version, prompt_free=True)
    vaux = _voice_args(4, 11, 5, version)
    vaux["refer_spec"] = vaux["refer_spec"] + [S.make_refer_spec(frames=41, seed=77).to(DEV)]
    if version == "v2Pro":
        vaux["sv_emb"] = vaux["sv_emb"] + [S.hash_symmetric("rb_sv_aux", (1, 20480), 1.0, 7).to(DEV)]
    reqs = [
        (va, dict(BASE, segments=_segs(0, [9, 5]), seed=3)),
        (va, dict(BASE, segments=_segs(1, [7]), seed=4)),                               # shares voice a
        (vb, dict(BASE, segments=_segs(2, [11, 6, 8]), batch_size=2, seed=5)),          # two batches of to_batch: two folds
        (vfree, dict(BASE, segments=_segs(3, [6, 9]), batch_size=2, seed=6)),           # prompt-free (AR side only): shared
        (vc, dict(BASE, segments=_segs(4, [10]), speed_factor=1.25, seed=7)),           # speed != 1: the per-request path
        (vaux, dict(BASE, segments=_segs(5, [8, 7]), batch_size=2, seed=8)),            # two reference spectrograms
    ]
    return va, vb, reqs


def _lsb(a, b):
    return int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max()) if a.size else 0


@pytest.mark.parametrize("version", ["v2", "v2Pro"])
def test_shared_pass_equals_run_per_request(version):
    """fp32.  decode_segments is held to 1e-5 of the isolated decode (test_each_segment_equals_its_isolated_decode_fp32), the
    generator ends in tanh so audio_postprocess never divides by a peak above 1, and 1e-5 * 32768 = 0.33 before
    truncation: at most 1 LSB per int16 sample."""
    tts = _build(version)
    va, vb, reqs = _mix(version)
    alone = [_alone(tts, kw, dict(req)) for kw, req in reqs]
    voices = {}
    for kw, _ in reqs:
        voices.setdefault(id(kw), tts.make_voice(**kw))
    tts.set_prompt_cache(**vb)
    cache = dict(tts.prompt_cache)
    batch = [dict(req, voice=voices[id(kw)]) for kw, req in reqs]
    n0 = tts.vits_model.decode_segments_calls
    out = tts.run_batch(batch, shared_sovits=True)
    assert tts.vits_model.decode_segments_calls - n0 == 1, "the shareable folds of the mix must take ONE shared pass"
    assert tts.prompt_cache.keys() == cache.keys() and all(tts.prompt_cache[k] is cache[k] for k in cache), \
        "run_batch changed the prompt cache"
    assert len(out) == len(reqs)
    for r, ((sr_a, a), (sr_b, b)) in enumerate(zip(alone, out)):
        assert sr_a == sr_b == 32000
        assert a.dtype == b.dtype == np.int16 and a.shape == b.shape, f"request {r}: {a.shape} vs {b.shape}"
        d = _lsb(a, b)
        print(f"{version} request {r}: max |shared - run()| = {d} LSB over {a.size} samples")
        assert d <= 1, f"request {r}: shared pass differs from run() alone by {d} LSB"
        assert np.abs(a).max() > 0
    assert np.array_equal(out[4][1], alone[4][1]), "the speed-1.25 request takes the per-request path: bit-equal"
    # the same text in two voices must sound different (a shared voice slot or a stale style vector would make them equal)
    seg = _segs(9, [8])
    two = tts.run_batch([dict(BASE, segments=seg, seed=1, voice=voices[id(va)]),
                         dict(BASE, segments=seg, seed=1, voice=voices[id(vb)])], shared_sovits=True)
    assert not np.array_equal(two[0][1], two[1][1])
    # run() after the shared pass still uses the prompt cache's voice
    assert np.array_equal(list(tts.run(dict(reqs[2][1])))[0][1], alone[2][1])


def test_frame_cap_splits_the_mix_into_two_passes():
    """sovits_max_frames one below the mix's frame count (gaps included): the same outputs through two passes"""
    tts = _build("v2")
    _, _, reqs = _mix("v2")
    alone = [_alone(tts, kw, dict(req)) for kw, req in reqs]
    batch = [dict(req, voice=tts.make_voice(**kw)) for kw, req in reqs]
    seen = []
    plan = tts.plan_sovits

    def spy(plans):
        launches = plan(plans)
        seen.append((launches, [[plans[r]["folds"][bi] for r, bi in L] for L in launches]))
        return launches
    tts.plan_sovits = spy
    n0 = tts.vits_model.decode_segments_calls
    one = tts.run_batch(batch, shared_sovits=True)
    launches, folds = seen[-1]
    assert tts.vits_model.decode_segments_calls - n0 == 1 and len(launches) == 1
    total = 2 * sum(folds[0]) + (len(folds[0]) - 1) * tts.vits_model.segment_gap()
    tts.sovits_max_frames = total - 1
    n0 = tts.vits_model.decode_segments_calls
    two = tts.run_batch(batch, shared_sovits=True)
    assert tts.vits_model.decode_segments_calls - n0 == 2 and len(seen[-1][0]) == 2
    for r, ((_, a), (_, b), (_, c)) in enumerate(zip(alone, one, two)):
        assert a.shape == b.shape == c.shape and _lsb(a, b) <= 1 and _lsb(a, c) <= 1, f"request {r}"


def test_shared_keyword_on_v3_changes_nothing():
    from test_pipeline_v3_gpu import _build as build_v3
    tts, *_ = build_v3("v3")
    vs = []
    for i, (P, n_ph, Tm) in enumerate([(8, 6, 26), (14, 4, 31)]):
        kw = _voice_args(10 + i, P, n_ph, "v3")
        kw["ref_mel"] = S.hash_symmetric(f"rb_mel{i}", (1, 100, Tm), 5.0, 3) - 5.0
        vs.append(kw)
    base = dict(top_k=5, sample_steps=2, fragment_interval=0.01)
    reqs = [(vs[0], dict(base, segments=_segs(20, [9, 6]), batch_size=2, seed=3)),
            (vs[1], dict(base, segments=_segs(21, [7]), seed=4))]
    batch = [dict(req, voice=tts.make_voice(**kw)) for kw, req in reqs]
    plain = tts.run_batch(batch)
    n0 = tts.vits_model.decode_segments_calls
    shared = tts.run_batch(batch, shared_sovits=True)
    assert tts.vits_model.decode_segments_calls == n0
    for (sr_a, a), (sr_b, b) in zip(plain, shared):
        assert sr_a == sr_b and a.shape == b.shape and np.array_equal(a, b)


def test_fp16_eight_voices_against_per_request_decodes():
    """fp16, 8 voices.  Both calls run the same AR launches and the engine is deterministic run to run, so the token counts
    (= output lengths) are equal; the waveforms differ only by segmented against isolated fp16 decode, held to the
    project's fp16 waveform bar (2e-2 of full scale max-abs, 3 % relative rms; test_production_shape_fp16)."""
    from gsv.TTS_infer_pack.TTS import TTS
    tcfg = S.small_t2s_config(n_layer=2, dim=128, head=4, vocab=1025, phoneme_vocab=732)
    tcfg["data"]["max_sec"] = 0.4
    tsd = S.make_t2s_state_dict(tcfg, seed=11, suppress_eos=False)
    vcfg = copy.deepcopy(S.small_vits_config())
    vsd = S.make_vits_state_dict(vcfg, seed=12)
    tts = TTS({"device": DEV, "is_half": True, "version": "v2", "max_batch": 8, "max_seq": 256})
    tts.init_t2s_weights(state={"weight": tsd, "config": tcfg})
    tts.init_vits_weights(state={"weight": vsd, "config": vcfg})
    batch = []
    for i in range(8):
        kw = _voice_args(20 + i, 6 + 3 * i, 4 + i % 3, "v2")
        kw["refer_spec"] = [s.half() for s in kw["refer_spec"]]
        batch.append(dict(BASE, segments=_segs(30 + i, [7 + i, 5 + (i % 4)]), batch_size=2, seed=10 + i, voice=tts.make_voice(**kw)))
    plain = tts.run_batch(batch)
    n0 = tts.vits_model.decode_segments_calls
    shared = tts.run_batch(batch, shared_sovits=True)
    assert tts.vits_model.decode_segments_calls - n0 == 1
    for r, ((_, a), (_, b)) in enumerate(zip(plain, shared)):
        assert a.shape == b.shape, f"request {r}: {a.shape} vs {b.shape} (token counts must be equal)"
    a = np.concatenate([x for _, x in plain]).astype(np.float64) / 32768.0
    b = np.concatenate([x for _, x in shared]).astype(np.float64) / 32768.0
    mx = float(np.abs(a - b).max())
    rel = float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(a ** 2)), 1e-12))
    print(f"fp16 8 voices: shared vs per-request max-abs {mx:.3e} of full scale, relative rms {rel:.3e}")
    assert mx <= 2e-2 and rel <= 3e-2
