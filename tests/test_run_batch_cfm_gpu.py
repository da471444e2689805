"""GPU: TTS.run_batch(shared_cfm=True) -- the flow-matching stage of all shareable v3 / v4 folds as rows of shared passes,
every row with its own voice's prompt -- against TTS.run per request (fp32) and against run_batch without it (fp16)."""
import numpy as np
import pytest
import torch

from gsv import synthetic as S
from test_pipeline_v3_gpu import _build as build_v3
from test_run_batch_gpu import _alone, _segs, _voice_args

pytestmark = pytest.mark.gpu

BASE = dict(top_k=5, sample_steps=2, fragment_interval=0.01)
BAR = 5e-3      # of full scale: the bar test_pipeline_v3_gpu.py sets for this fragment path against its reference


def _voice(i, P, n_ph, Tm, version):
    kw = _voice_args(10 + i, P, n_ph, version)
    kw["ref_mel"] = S.hash_symmetric(f"rbc_mel{i}", (1, 100, Tm), 5.0, 3) - 5.0
    return kw


def _mix(version):
    """three voices whose prompts are 14, 20 (31 cut to T_ref) and 17 frames; five requests"""
    va, vb, vc = _voice(0, 8, 6, 14, version), _voice(1, 14, 4, 31, version), _voice(2, 11, 7, 17, version)
    reqs = [(va, dict(BASE, segments=_segs(20, [9, 5]), batch_size=2, seed=3)),
            (va, dict(BASE, segments=_segs(21, [7]), seed=4)),                                   # shares voice a
            (vb, dict(BASE, segments=_segs(22, [11, 6, 8]), batch_size=2, seed=5)),              # two to_batch batches: two folds
            (vc, dict(BASE, segments=_segs(23, [6]), parallel_infer=False, seed=6)),             # chunk by chunk: per request
            (vc, dict(BASE, segments=_segs(24, [10]), speed_factor=1.25, seed=7))]               # speed only enters decode_encp
    return va, vb, reqs


def _diff(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) / 32768.0 if a.size else 0.0


def _spy(tts):
    """count CFM.inference_rows calls and their rows"""
    cfm, calls = tts.vits_model.cfm, []
    inner = cfm.inference_rows

    def wrapped(mu, prompts, *a, **k):
        calls.append((int(mu.shape[0]), sorted({int(p.shape[2]) for p in prompts})))
        return inner(mu, prompts, *a, **k)
    cfm.inference_rows = wrapped
    return calls


@pytest.mark.parametrize("version", ["v3", "v4"])
def test_shared_cfm_equals_run_per_request(version):
    """fp32.  Every request of the mix against run() alone: equal int16 shapes (equal SOLA offsets) and samples within 5e-3
    of full scale; the non-parallel request bit-equal; one inference_rows call for the mix; prompt cache untouched; run()
    afterwards unchanged; the same text in two voices differs."""
    tts, *_ = build_v3(version)
    va, vb, reqs = _mix(version)
    alone = [_alone(tts, kw, dict(req)) for kw, req in reqs]
    voices = {}
    for kw, _ in reqs:
        voices.setdefault(id(kw), tts.make_voice(**kw))
    tts.set_prompt_cache(**vb)
    cache = dict(tts.prompt_cache)
    batch = [dict(req, voice=voices[id(kw)]) for kw, req in reqs]
    calls = _spy(tts)
    out = tts.run_batch(batch, shared_cfm=True)
    assert len(calls) == 1, f"the shareable folds of the mix must take ONE flow-matching pass, got {calls}"
    assert calls[0][0] >= 5 and len(calls[0][1]) == 3, f"rows of three prompt lengths in the pass, got {calls[0]}"
    assert tts.prompt_cache.keys() == cache.keys() and all(tts.prompt_cache[k] is cache[k] for k in cache), \
        "run_batch changed the prompt cache"
    assert len(out) == len(reqs)
    for r, ((sr_a, a), (sr_b, b)) in enumerate(zip(alone, out)):
        assert sr_a == sr_b
        assert a.dtype == b.dtype == np.int16 and a.shape == b.shape, f"request {r}: {a.shape} vs {b.shape}"
        d = _diff(a, b)
        print(f"{version} request {r}: max |shared - run()| = {d:.3e} of full scale over {a.size} samples")
        assert d <= BAR, f"request {r}: shared pass differs from run() alone by {d:.3e} of full scale"
        assert np.abs(a).max() > 0
    assert np.array_equal(out[3][1], alone[3][1]), "the parallel_infer=False request takes the per-request path: bit-equal"
    seg = _segs(29, [8])
    two = tts.run_batch([dict(BASE, segments=seg, seed=1, voice=voices[id(va)]),
                         dict(BASE, segments=seg, seed=1, voice=voices[id(vb)])], shared_cfm=True)
    assert two[0][1].shape != two[1][1].shape or not np.array_equal(two[0][1], two[1][1])
    assert np.array_equal(list(tts.run(dict(reqs[2][1])))[0][1], alone[2][1]), "run() after the shared pass"


def test_row_cap_splits_the_mix_into_two_passes():
    """cfm_max_rows one below the mix's row count: two passes, every output within the same bar of the one-pass result"""
    tts, *_ = build_v3("v3")
    _, _, reqs = _mix("v3")
    batch = [dict(req, voice=tts.make_voice(**kw)) for kw, req in reqs]
    calls = _spy(tts)
    one = tts.run_batch(batch, shared_cfm=True)
    assert len(calls) == 1
    total = calls[0][0]
    assert 2 <= total <= tts.cfm_max_rows
    tts.cfm_max_rows = total - 1
    del calls[:]
    two = tts.run_batch(batch, shared_cfm=True)
    assert [n for n, _ in calls] == [total - 1, 1]
    for r, ((_, a), (_, b)) in enumerate(zip(one, two)):
        assert a.shape == b.shape, f"request {r}"
        d = _diff(a, b)
        print(f"request {r}: max |two passes - one pass| = {d:.3e} of full scale")
        assert d <= BAR


def test_fp16_eight_voices_against_per_request_passes():
    """fp16, 8 voices: shared_cfm=True against run_batch().  Both run the same AR launches, so the token counts are equal;
    the project's fp16 vocoder bar over all requests: 3e-2 max-abs of full scale, 5 % relative RMS."""
    tts, *_ = build_v3("v3", is_half=True)
    batch = []
    for i in range(8):
        kw = _voice(20 + i, 6 + 2 * i, 4 + i % 3, 12 + 3 * i, "v3")
        batch.append(dict(BASE, segments=_segs(40 + i, [7 + i, 5 + (i % 4)]), batch_size=2, seed=10 + i, voice=tts.make_voice(**kw)))
    plain = tts.run_batch(batch)
    calls = _spy(tts)
    shared = tts.run_batch(batch, shared_cfm=True)
    assert len(calls) >= 1 and sum(n for n, _ in calls) >= 8
    for r, ((_, a), (_, b)) in enumerate(zip(plain, shared)):
        assert a.shape == b.shape, f"request {r}: {a.shape} vs {b.shape}"
    a = np.concatenate([x for _, x in plain]).astype(np.float64) / 32768.0
    b = np.concatenate([x for _, x in shared]).astype(np.float64) / 32768.0
    mx = float(np.abs(a - b).max())
    rel = float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(a ** 2)), 1e-12))
    print(f"fp16 8 voices: shared vs per-request max-abs {mx:.3e} of full scale, relative rms {rel:.3e}")
    assert mx <= 3e-2 and rel <= 5e-2


def test_shared_cfm_on_v2_changes_nothing():
    from test_run_batch_gpu import _build
    tts = _build("v2")
    reqs = [(_voice_args(0, 8, 6, "v2"), dict(top_k=5, fragment_interval=0.01, segments=_segs(0, [9, 5]), seed=3)),
            (_voice_args(1, 23, 4, "v2"), dict(top_k=5, fragment_interval=0.01, segments=_segs(2, [11, 6]), batch_size=2, seed=5))]
    batch = [dict(req, voice=tts.make_voice(**kw)) for kw, req in reqs]
    plain = tts.run_batch(batch)
    shared = tts.run_batch(batch, shared_cfm=True)
    for (sr_a, a), (sr_b, b) in zip(plain, shared):
        assert sr_a == sr_b and a.shape == b.shape and np.array_equal(a, b)
