"""GPU: the request key `inference_cfg_rate` through TTS.run and TTS.run_batch(shared_cfm=True) on the small synthetic v3 / v4
models of test_run_batch_cfm_gpu.py, fp32: guided requests of several voices share a guided flow-matching pass, unguided
ones keep theirs, and every request equals its own run()."""
import numpy as np
import pytest

from test_pipeline_v3_gpu import _build as build_v3
from test_run_batch_cfm_gpu import BAR, BASE, _diff, _voice
from test_run_batch_gpu import _alone, _segs

pytestmark = pytest.mark.gpu
RATE = 0.7


def _spy(tts):
    """(rows, guidance rate) of every CFM.inference_rows call"""
    cfm, calls = tts.vits_model.cfm, []
    inner = cfm.inference_rows

    def wrapped(mu, prompts, *a, **k):
        calls.append((int(mu.shape[0]), k.get("inference_cfg_rate", 0)))
        return inner(mu, prompts, *a, **k)
    cfm.inference_rows = wrapped
    return calls


@pytest.mark.parametrize("version", ["v3", "v4"])
def test_run_takes_the_rate(version):
    """run() with inference_cfg_rate = 0.7: the sample count of rate 0 (the AR decode and the SOLA cuts do not see the rate)
    and different audio, on the batched and on the chunk-by-chunk path; a rate at or below 1e-5 is rate 0, bit for bit"""
    tts, *_ = build_v3(version)
    va = _voice(0, 8, 6, 14, version)
    for extra in ({}, {"parallel_infer": False}):
        req = dict(BASE, segments=_segs(20, [9, 5]), batch_size=2, seed=3, **extra)
        sr0, plain = _alone(tts, va, dict(req))
        sr1, guided = _alone(tts, va, dict(req, inference_cfg_rate=RATE))
        assert sr0 == sr1 and plain.dtype == guided.dtype == np.int16 and plain.shape == guided.shape
        assert np.abs(guided).max() > 0
        d = _diff(plain, guided)
        print(f"{version} {extra}: max |guided - unguided| = {d:.3e} of full scale over {plain.size} samples")
        assert d > BAR, "the rate changed nothing audible"
        assert np.array_equal(_alone(tts, va, dict(req, inference_cfg_rate=1e-6))[1], plain)
        assert np.array_equal(_alone(tts, va, dict(req, inference_cfg_rate=RATE))[1], guided)


@pytest.mark.parametrize("version", ["v3", "v4"])
def test_shared_cfm_guided_requests_of_two_voices_and_one_unguided(version):
    """run_batch(shared_cfm=True) over guided requests of two voices (three requests) plus one unguided request: every
    request within 5e-3 of full scale of its own run() with equal sample counts; the passes are as planned -- the guided
    rows of both voices together, cfm_max_rows // 2 to a pass, the unguided request's rows in one pass of their own, where
    its guided neighbours cannot reach it: its output is the one it has in a batch without them."""
    tts, *_ = build_v3(version)
    va, vb = _voice(0, 8, 6, 14, version), _voice(1, 14, 4, 31, version)
    reqs = [(va, dict(BASE, segments=_segs(20, [9, 5]), batch_size=2, seed=3, inference_cfg_rate=RATE)),
            (vb, dict(BASE, segments=_segs(22, [11, 6, 8]), batch_size=2, seed=5, inference_cfg_rate=RATE)),   # two folds
            (va, dict(BASE, segments=_segs(21, [7]), seed=4)),                                                # unguided
            (vb, dict(BASE, segments=_segs(23, [6]), seed=6, inference_cfg_rate=RATE))]
    alone = [_alone(tts, kw, dict(req)) for kw, req in reqs]
    voices = {}
    for kw, _ in reqs:
        voices.setdefault(id(kw), tts.make_voice(**kw))
    batch = [dict(req, voice=voices[id(kw)]) for kw, req in reqs]
    calls = _spy(tts)
    out = tts.run_batch(batch, shared_cfm=True)
    guided, plain = [n for n, rate in calls if rate > 1e-5], [n for n, rate in calls if not rate > 1e-5]
    half = tts.cfm_max_rows // 2
    assert all(rate == RATE for _, rate in calls if rate > 1e-5) and sum(guided) >= 4, calls
    assert guided == [half] * (sum(guided) // half) + [sum(guided) % half] * (sum(guided) % half > 0), \
        f"the guided rows of both voices fill passes of cfm_max_rows // 2 = {half} rows, got {calls}"
    assert len(plain) == 1 and plain[0] >= 1, f"one pass for the unguided request, got {calls}"
    for r, ((sr_a, a), (sr_b, b)) in enumerate(zip(alone, out)):
        assert sr_a == sr_b
        assert a.dtype == b.dtype == np.int16 and a.shape == b.shape, f"request {r}: {a.shape} vs {b.shape}"
        d = _diff(a, b)
        print(f"{version} request {r}: max |shared - run()| = {d:.3e} of full scale ({d * 32768:.1f} LSB) over {a.size} samples")
        assert d <= BAR, f"request {r}: shared pass differs from run() alone by {d:.3e} of full scale"
        assert np.abs(a).max() > 0
    del calls[:]
    only = tts.run_batch([batch[2]], shared_cfm=True)
    assert len(calls) == 1 and not calls[0][1] > 1e-5
    assert np.array_equal(only[0][1], out[2][1]), "the unguided request changed with its guided neighbours"
    # a guided cap of one row: every guided row its own pass, the same audio within the bar
    tts.cfm_max_rows = 2
    del calls[:]
    split = tts.run_batch(batch, shared_cfm=True)
    assert all(n == 1 for n, rate in calls if rate > 1e-5) and all(n <= 2 for n, _ in calls)
    for r, ((_, a), (_, b)) in enumerate(zip(out, split)):
        assert a.shape == b.shape and _diff(a, b) <= BAR, f"request {r}"
