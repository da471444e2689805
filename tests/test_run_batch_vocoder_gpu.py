"""GPU: TTS.run_batch(shared_cfm=True, shared_vocoder=True) -- the folds of the shared flow-matching stage vocoded in shared
segmented passes over all voices -- against run_batch(shared_cfm=True), which vocodes one fold per call.  The mix is the one of
tests/test_run_batch_cfm_gpu.py: five requests over three voices, small v3 and v4 models."""
import numpy as np
import pytest

from gsv import synthetic as S
from test_pipeline_v3_gpu import _build as build_v3
from test_run_batch_gpu import _segs, _voice_args

pytestmark = pytest.mark.gpu

BASE = dict(top_k=5, sample_steps=2, fragment_interval=0.01)
BAR = 5e-3      # of full scale: the bar tests/test_run_batch_cfm_gpu.py sets for the shared flow-matching stage


def _voice(i, P, n_ph, Tm, version):
    kw = _voice_args(10 + i, P, n_ph, version)
    kw["ref_mel"] = S.hash_symmetric(f"rbc_mel{i}", (1, 100, Tm), 5.0, 3) - 5.0
    return kw


def _mix(version):
    """three voices whose prompts are 14, 20 (31 cut to T_ref) and 17 frames; five requests"""
    va, vb, vc = _voice(0, 8, 6, 14, version), _voice(1, 14, 4, 31, version), _voice(2, 11, 7, 17, version)
    return [(va, dict(BASE, segments=_segs(20, [9, 5]), batch_size=2, seed=3)),
            (va, dict(BASE, segments=_segs(21, [7]), seed=4)),                                   # shares voice a
            (vb, dict(BASE, segments=_segs(22, [11, 6, 8]), batch_size=2, seed=5)),              # two to_batch batches: two folds
            (vc, dict(BASE, segments=_segs(23, [6]), parallel_infer=False, seed=6)),             # chunk by chunk: per request
            (vc, dict(BASE, segments=_segs(24, [10]), speed_factor=1.25, seed=7))]               # speed only enters decode_encp


def _batch(tts, reqs):
    voices = {}
    for kw, _ in reqs:
        voices.setdefault(id(kw), tts.make_voice(**kw))
    return [dict(req, voice=voices[id(kw)]) for kw, req in reqs]


def _diff(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) / 32768.0 if a.size else 0.0


def _spy(tts):
    """the frame counts of every forward_segments call"""
    voc, calls = tts.vocoder, []
    inner = voc.forward_segments

    def wrapped(mels):
        calls.append([int(m.shape[2]) for m in mels])
        return inner(mels)
    voc.forward_segments = wrapped
    return calls


@pytest.mark.parametrize("version", ["v3", "v4"])
def test_shared_vocoder_equals_the_per_fold_vocoder(version):
    """fp32.  One forward_segments pass for the mix (the folds of its four parallel_infer requests); every request has the
    int16 shape run_batch(shared_cfm=True) gives it (equal SOLA offsets) and samples within 5e-3 of full scale; the
    parallel_infer=False request is bit-equal to the call without the keyword; with vocoder_max_frames one below the total:
    two passes, the same audio within the bar."""
    tts, *_ = build_v3(version)
    batch = _batch(tts, _mix(version))
    plain = tts.run_batch(batch, shared_cfm=True)
    calls = _spy(tts)
    shared = tts.run_batch(batch, shared_cfm=True, shared_vocoder=True)
    assert len(calls) == 1, f"the folds of the mix must take ONE vocoder pass, got {calls}"
    one = list(calls[0])
    assert len(one) >= 4, f"the folds of four requests, r2 with two of them, got {one}"
    for r, ((sr_a, a), (sr_b, b)) in enumerate(zip(plain, shared)):
        assert sr_a == sr_b and a.dtype == b.dtype == np.int16 and a.shape == b.shape, f"request {r}: {a.shape} vs {b.shape}"
        d = _diff(a, b)
        print(f"{version} request {r}: max |shared vocoder - per fold| = {d:.3e} of full scale over {a.size} samples")
        assert d <= BAR and np.abs(b).max() > 0
    assert np.array_equal(shared[3][1], plain[3][1]), "the parallel_infer=False request takes the per-request path: bit-equal"
    total = sum(one)
    assert total <= tts.vocoder_max_frames
    tts.vocoder_max_frames = total - 1
    del calls[:]
    two = tts.run_batch(batch, shared_cfm=True, shared_vocoder=True)
    assert len(calls) == 2 and calls[0] + calls[1] == one and calls[1] == one[-1:], f"two passes over the same folds, got {calls}"
    for r, ((_, a), (_, b)) in enumerate(zip(plain, two)):
        assert a.shape == b.shape, f"request {r}"
        d = _diff(a, b)
        print(f"{version} request {r}: max |two passes - per fold| = {d:.3e} of full scale")
        assert d <= BAR


def test_fp16_eight_voices_against_the_per_fold_vocoder():
    """fp16, 8 voices: shared_vocoder=True against run_batch(shared_cfm=True); the project's fp16 vocoder bar over all requests:
    3e-2 max-abs of full scale, 5 % relative RMS"""
    tts, *_ = build_v3("v3", is_half=True)
    batch = []
    for i in range(8):
        kw = _voice(20 + i, 6 + 2 * i, 4 + i % 3, 12 + 3 * i, "v3")
        batch.append(dict(BASE, segments=_segs(40 + i, [7 + i, 5 + (i % 4)]), batch_size=2, seed=10 + i, voice=tts.make_voice(**kw)))
    plain = tts.run_batch(batch, shared_cfm=True)
    calls = _spy(tts)
    shared = tts.run_batch(batch, shared_cfm=True, shared_vocoder=True)
    assert len(calls) == 1 and len(calls[0]) >= 8
    for r, ((_, a), (_, b)) in enumerate(zip(plain, shared)):
        assert a.shape == b.shape, f"request {r}: {a.shape} vs {b.shape}"
    a = np.concatenate([x for _, x in plain]).astype(np.float64) / 32768.0
    b = np.concatenate([x for _, x in shared]).astype(np.float64) / 32768.0
    mx = float(np.abs(a - b).max())
    rel = float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(a ** 2)), 1e-12))
    print(f"fp16 8 voices: shared vocoder vs per fold max-abs {mx:.3e} of full scale, relative rms {rel:.3e}")
    assert mx <= 3e-2 and rel <= 5e-2


def test_value_error_without_shared_cfm_and_v2_is_unaffected():
    tts, *_ = build_v3("v3")
    batch = _batch(tts, _mix("v3")[:1])
    with pytest.raises(ValueError):
        tts.run_batch(batch, shared_vocoder=True)
    from test_run_batch_gpu import _build
    v2 = _build("v2")
    reqs = [(_voice_args(0, 8, 6, "v2"), dict(top_k=5, fragment_interval=0.01, segments=_segs(0, [9, 5]), seed=3)),
            (_voice_args(1, 23, 4, "v2"), dict(top_k=5, fragment_interval=0.01, segments=_segs(2, [11, 6]), batch_size=2, seed=5))]
    batch = [dict(req, voice=v2.make_voice(**kw)) for kw, req in reqs]
    for (sr_a, a), (sr_b, b) in zip(v2.run_batch(batch), v2.run_batch(batch, shared_vocoder=True)):
        assert sr_a == sr_b and a.shape == b.shape and np.array_equal(a, b)
