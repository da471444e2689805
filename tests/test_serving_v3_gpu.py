"""GPU: gsv.serving.Scheduler on the fp32 small v3 pipeline of test_pipeline_v3_gpu.py: two requests with different voices that
arrive one step apart take their flow-matching stage from _shared_cfm_stage -- in two waves, or in one when wave_hold lets the
first wait for the second -- and each is what run_batch([request]) alone returns: the same AR tokens, audio of the same shape
within 1 int16 LSB."""
import numpy as np
import pytest

from gsv.serving import Scheduler, plan_online
from test_pipeline_v3_gpu import _build as build_v3
from test_run_batch_cfm_gpu import BASE, _spy as _cfm_calls, _voice
from test_run_batch_continuous_gpu import _run_batch
from test_run_batch_gpu import _segs
from test_run_batch_shared_gpu import _lsb
from test_serving_gpu import _spy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    tts, *_ = build_v3("v3")
    va, vb = _voice(0, 8, 6, 14, "v3"), _voice(1, 14, 4, 31, "v3")
    batch = [dict(BASE, segments=_segs(20, [9, 5]), batch_size=2, seed=3, voice=tts.make_voice(**va)),
             dict(BASE, segments=_segs(22, [11, 6, 8]), batch_size=2, seed=5, voice=tts.make_voice(**vb))]
    alone = []
    for req in batch:
        out, preds = _run_batch(tts, [req])
        alone.append((out[0][0], out[0][1], preds[0]))
        assert np.abs(out[0][1]).max() > 0
    return tts, batch, alone, _cfm_calls(tts)


@pytest.mark.parametrize("wave_hold, waves", [(0, [[0], [1]]), (8, [[0, 1]])])
def test_two_voices_one_step_apart(world, wave_hold, waves):
    tts, batch, alone, calls = world
    results = {}
    del calls[:]
    with _spy(tts) as (seen, _), Scheduler(tts, chunk=8, wave_hold=wave_hold) as sched:
        for req in batch:
            sched.submit(req)
            results.update(sched.step())
        n = 0
        while not sched.idle:
            results.update(sched.step())
            n += 1
            assert n <= 40
        stats = sched.stats
    lengths = [i for r in range(2) for idx in seen[batch[r]["seed"]][1] for i in idx]
    plan = plan_online([0, 1], [2, 3], lengths, slots=4, chunk=8, wave_hold=wave_hold)
    assert stats["events"] == plan
    assert [e[1] for e in plan if e[0] == "wave"] == waves and stats["waves"] == len(waves)
    assert len(calls) == len(waves), f"one flow-matching pass per wave, got {calls}"
    if len(waves) == 1:
        assert len(calls[0][1]) == 2, f"rows of both voices' prompt lengths share the pass, got {calls[0]}"
    for r in range(2):
        sr, audio, tokens = alone[r]
        assert not isinstance(results[r], BaseException), results[r]
        assert seen[batch[r]["seed"]][0] == tokens, f"request {r}: other tokens than in run_batch([request])"
        got_sr, got = results[r]
        assert got_sr == sr and got.dtype == np.int16 and got.shape == audio.shape
        print(f"v3 request {r}, wave_hold {wave_hold}: {_lsb(got, audio)} LSB from run_batch([request]) over {got.size} samples")
        assert _lsb(got, audio) <= 1, f"request {r}: {_lsb(got, audio)} LSB from run_batch([request])"
