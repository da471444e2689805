"""GPU: TTS.run_batch(shared_sovits=True, shared_speed=True) -- the sentences of requests at speed_factor != 1 in the same
segmented SoVITS pass as the speed-1 folds -- against TTS.run per request (fp32: at most 1 LSB of the int16 output), and
the keyword left off or on a v3 model changing nothing."""
import numpy as np
import pytest

from gsv import synthetic as S
from test_run_batch_gpu import _alone, _build, _segs, _voice_args
from test_run_batch_shared_gpu import BASE, _lsb, _mix

pytestmark = pytest.mark.gpu


def _mix_speed(version):
    """the six requests of the shared-pass mix (one at speed 1.25) plus a slowed-down one with two sentences"""
    va, vb, reqs = _mix(version)
    reqs = reqs + [(va, dict(BASE, segments=_segs(6, [7, 10]), speed_factor=0.8, seed=9))]
    return va, vb, reqs


def _batch(tts, reqs):
    voices = {}
    for kw, _ in reqs:
        voices.setdefault(id(kw), tts.make_voice(**kw))
    return [dict(req, voice=voices[id(kw)]) for kw, req in reqs]


@pytest.mark.parametrize("version", ["v2", "v2Pro"])
def test_shared_speed_pass_equals_run_per_request(version):
    """fp32.  A segment at any speed is held to 1e-5 of its isolated decode (test_vits_segments_speed_gpu), the generator
    ends in tanh so audio_postprocess never divides by a peak above 1, and 1e-5 * 32768 = 0.33 before truncation: at most
    1 LSB per int16 sample, as for the speed-1 shared pass."""
    tts = _build(version)
    va, vb, reqs = _mix_speed(version)
    alone = [_alone(tts, kw, dict(req)) for kw, req in reqs]
    batch = _batch(tts, reqs)
    tts.set_prompt_cache(**vb)
    cache = dict(tts.prompt_cache)
    n0 = tts.vits_model.decode_segments_calls
    out = tts.run_batch(batch, shared_sovits=True, shared_speed=True)
    assert tts.vits_model.decode_segments_calls - n0 == 1, "folds and speed sentences of the mix must take ONE shared pass"
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
    # keyword off: the speed requests stay on the per-request path, bit-equal to run() alone
    n0 = tts.vits_model.decode_segments_calls
    off = tts.run_batch(batch, shared_sovits=True)
    assert tts.vits_model.decode_segments_calls - n0 == 1
    for r in (4, 6):
        assert np.array_equal(off[r][1], alone[r][1]), f"request {r} (speed != 1) without shared_speed: not bit-equal to run()"
    # shared_speed alone (no shared_sovits) is run_batch as it was: no segmented pass at all
    n0 = tts.vits_model.decode_segments_calls
    plain = tts.run_batch(batch, shared_speed=True)
    assert tts.vits_model.decode_segments_calls == n0
    for r, ((_, a), (_, b)) in enumerate(zip(alone, plain)):
        assert np.array_equal(a, b), f"request {r}"


def test_shared_speed_keyword_on_v3_changes_nothing():
    from test_pipeline_v3_gpu import _build as build_v3
    tts, *_ = build_v3("v3")
    vs = []
    for i, (P, n_ph, Tm) in enumerate([(8, 6, 26), (14, 4, 31)]):
        kw = _voice_args(10 + i, P, n_ph, "v3")
        kw["ref_mel"] = S.hash_symmetric(f"rb_mel{i}", (1, 100, Tm), 5.0, 3) - 5.0
        vs.append(kw)
    base = dict(top_k=5, sample_steps=2, fragment_interval=0.01)
    reqs = [(vs[0], dict(base, segments=_segs(20, [9, 6]), batch_size=2, seed=3)),
            (vs[1], dict(base, segments=_segs(21, [7]), speed_factor=1.25, seed=4))]
    batch = [dict(req, voice=tts.make_voice(**kw)) for kw, req in reqs]
    plain = tts.run_batch(batch)
    n0 = tts.vits_model.decode_segments_calls
    shared = tts.run_batch(batch, shared_sovits=True, shared_speed=True)
    assert tts.vits_model.decode_segments_calls == n0
    for (sr_a, a), (sr_b, b) in zip(plain, shared):
        assert sr_a == sr_b and a.shape == b.shape and np.array_equal(a, b)
