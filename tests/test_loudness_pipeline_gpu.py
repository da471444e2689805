"""GPU: the request keys "loudness", "loudness_scope" and "loudness_peak"  through run, its fragments,
run_batch, the server and the wire handler, on the fp32 small v2 and v3 pipelines of test_output_format_pipeline_gpu.py.

The default result q is the truncation of the waveform x * 32768, the loud result that of g * x * 32768 (the gain multiplies the
same fp32 sample): |loud - g q| <= g + 1 LSB per sample.  The meter reads x, the mirror q / 32768, which differ by less than one
LSB per sample: with r the rms in LSB of the lowest gated block, the two levels differ by at most 20 log10(1 + 1 / r) LU."""
import math

import numpy as np
import pytest

import _loudness_ref as R
from gsv import audio_io, wire
from gsv.serving import Scheduler
from test_output_format_pipeline_gpu import _meets, _one, _peaks, _v3_req
from test_run_batch_gpu import _build, _segs, _voice_args
from test_run_batch_shared_gpu import BASE, _lsb
from test_serving_stream_gpu import _drive, _run_stream

pytestmark = pytest.mark.gpu
WAIT = 120.0
TARGET = -20.0


@pytest.fixture(scope="module")
def v2():
    tts = _build("v2")
    tts.set_prompt_cache(**_voice_args(0, 8, 6, "v2"))
    return tts


@pytest.fixture(scope="module")
def v3():
    from test_audio_sr_gpu import _tts_with_sr
    return _tts_with_sr("v3")


def _v2_req():
    return dict(BASE, segments=_segs(60, [9, 5, 7]), batch_size=2, seed=3)


def _scaled(loud, q, g):
    """the largest |loud - g q| in LSB"""
    return float(np.abs(loud.astype(np.float64) - g * q.astype(np.float64)).max()) if q.size else 0.0


def _level_bar(q, rate):
    """(the mirror's level of q / 32768, the allowed distance to the device's, r)"""
    m = R.meter(q.astype(np.float64) / 32768.0, rate)
    assert m["rel"].any(), "the default result is gated out: choose another text"
    r = math.sqrt(float(m["z"][m["rel"]].min())) * 32768.0
    return m["lufs"], 20.0 * math.log10(1.0 + 1.0 / r), r


@pytest.mark.parametrize("model", ["v2", "v3"])
def test_run_with_loudness(model, request):
    tts = request.getfixturevalue(model)
    req, sr0 = (_v2_req(), 32000) if model == "v2" else (_v3_req(), 24000)
    peaks = _peaks(tts, 1.0 if model == "v2" else 0.5)
    try:
        sr, q = _one(tts, req)
        assert sr == sr0 and peaks and max(peaks) < 1.0, "a sentence is normalised or wraps: q is then not the truncated waveform"
        assert tts.last_loudness == []
        sr, a = _one(tts, dict(req, loudness=TARGET))
        assert sr == sr0 and a.dtype == np.int16 and a.shape == q.shape
        assert len(tts.last_loudness) == 1 and len(tts.last_loudness[0]) == 1
        rep = tts.last_loudness[0][0]
        g = rep["gain"]
        assert g != 1.0 and rep["gain_db"] == pytest.approx(20.0 * math.log10(g))
        worst = _scaled(a, q, g)
        lufs, bar, r = _level_bar(q, sr0)
        print(f"\n{model}: gain {g:.4f}, {worst:.2f} LSB from g q (bar {g + 1:.2f}); {rep['lufs']:.4f} LUFS, mirror {lufs:.4f}, "
              f"bar {bar:.4f} LU, r = {r:.0f} LSB")
        assert worst <= g + 1.0
        assert r >= 100.0
        assert abs(rep["lufs"] - lufs) <= bar
        if not rep["limited"]:
            assert abs(rep["lufs"] + rep["gain_db"] - TARGET) <= 1e-4
        # sentence scope: one report per sentence, each sentence under its own gain
        sr, b = _one(tts, dict(req, loudness=TARGET, loudness_scope="sentence"))
        lens = list(tts.last_fragment_lengths)
        reps = tts.last_loudness[0]
        assert len(tts.last_loudness) == 1 and len(reps) == len(lens) >= 2 and sum(lens) == len(q) == len(b)
        at = 0
        for n, rp in zip(lens, reps):
            assert _scaled(b[at:at + n], q[at:at + n], rp["gain"]) <= rp["gain"] + 1.0
            at += n
        assert len({rp["gain"] for rp in reps}) > 1
    finally:
        del tts.audio_postprocess


def test_other_rate_and_encoding_with_loudness(v2):
    req = _v2_req()
    sr, a = _one(v2, dict(req, loudness=TARGET))
    got = _one(v2, dict(req, loudness=TARGET, sample_rate=8000, encoding="mulaw"))
    want = (8000, audio_io.convert_pcm(a, 32000, 8000, "mulaw"))
    _meets(got, want, {"sample_rate": 8000, "encoding": "mulaw"}, "loudness with 8 kHz mu-law")


def test_every_fragment_is_normalised_on_its_own(v2):
    req = _v2_req()
    plain = list(v2.run(dict(req, return_fragment=True)))
    frags = list(v2.run(dict(req, return_fragment=True, loudness=TARGET, loudness_peak=-1.0)))
    assert len(frags) == len(plain) == 2 and len(v2.last_loudness) == 2
    ceiling = 10.0 ** (-1.0 / 20.0) * 32768.0
    for (sr, a), (_, q), reps in zip(frags, plain, v2.last_loudness):
        assert len(reps) == 1 and _scaled(a, q, reps[0]["gain"]) <= reps[0]["gain"] + 1.0
        assert np.abs(a.astype(np.int32)).max() <= ceiling + 1.0


def test_server_with_and_without_loudness(v2):
    kws = [_voice_args(0, 8, 6, "v2"), _voice_args(1, 23, 4, "v2")]
    voices = [v2.make_voice(**kw) for kw in kws]
    reqs = [dict(BASE, segments=_segs(61, [9, 5, 7]), batch_size=2, seed=3, voice=voices[0], loudness=TARGET),
            dict(BASE, segments=_segs(62, [7, 12]), batch_size=2, seed=4, voice=voices[1])]
    alone = [v2.run_batch([dict(r)])[0] for r in reqs[:1]]
    g = v2.last_loudness[0][0]["gain"]
    alone.append(v2.run_batch([dict(reqs[1])])[0])
    assert v2.last_loudness == []
    server = v2.serve(slots=4, chunk=4)
    try:
        futs = [server.submit(dict(r)) for r in reqs]
        got = [f.result(timeout=WAIT) for f in futs]
        assert len(v2.last_loudness) <= 1                                   # the last post-processing call's, not a log
        more = [server.submit(dict(reqs[0], seed=10 + i)) for i in range(3)]
        assert not any(isinstance(f.result(timeout=WAIT), BaseException) for f in more)
        assert len(v2.last_loudness) <= 1, "last_loudness grows with the number of served requests"
    finally:
        server.shutdown(timeout=WAIT)
    assert server.error is None
    for i in range(2):
        assert not isinstance(got[i], BaseException), got[i]
        assert got[i][0] == alone[i][0] == 32000 and got[i][1].shape == alone[i][1].shape
    assert _lsb(got[1][1], alone[1][1]) <= 1                                # the plain request: the server's bar on the parent path
    assert _lsb(got[0][1], alone[0][1]) <= math.ceil(g) + 1


def test_one_postprocessing_call_per_step(v2):
    """streams with and without loudness, other targets and scopes, all in the default format: _emit makes one call per step"""
    kws = [_voice_args(0, 8, 6, "v2"), _voice_args(1, 23, 4, "v2"), _voice_args(2, 5, 7, "v2")]
    voices = [v2.make_voice(**kw) for kw in kws]
    extra = [dict(loudness=TARGET), dict(loudness=-16.0, loudness_scope="sentence", loudness_peak=-1.0), {}]
    batch = [dict(BASE, segments=_segs(61 + i, lens), batch_size=2, seed=3 + i, voice=voices[i], return_fragment=True, **extra[i])
             for i, lens in enumerate([[9, 5, 7], [7, 12], [11, 6, 8]])]
    inner, calls, per_emit, reports = v2.postprocess_fragments, [], [], []

    def counted(groups, **kw):
        calls.append(kw.get("loudness"))
        out = inner(groups, **kw)
        if kw.get("loudness") is not None:
            reports.append(list(v2.last_loudness))
        return out
    v2.postprocess_fragments = counted
    results, plans, frag_steps = {}, {}, {}
    try:
        with Scheduler(v2, slots=4, chunk=32) as sched:
            emit = sched._emit

            def emitting(due, ends):
                before = len(calls)
                out = emit(due, ends)
                per_emit.append((len(calls) - before, len(out)))
                return out
            sched._emit = emitting
            _drive(sched, batch, [[0, 1, 2]], plans, results, frag_steps)
    finally:
        del v2.postprocess_fragments
    assert all(isinstance(results[r], list) and len(results[r]) == (2, 1, 2)[r] for r in range(3)), results   # folds of two sentences
    assert len(v2.last_loudness) <= 2                                       # the last call's fragments, not every step's
    # the plain stream shared its calls with loud fragments: the same audio as run()'s fragments, the server's bar (it leaves
    # through the saturating conversion there, which differs from the wrapping one only at +1.0 and beyond)
    plain = {k: v for k, v in batch[2].items() if k not in ("return_fragment", "voice")}
    want, _ = _run_stream(v2, kws[2], plain)
    assert len(want) == len(results[2])
    for (sr_g, g), (sr_w, w) in zip(results[2], want):
        assert sr_g == sr_w == 32000 and g.dtype == np.int16 and g.shape == w.shape and _lsb(g, w) <= 1
    assert per_emit and all(n_calls <= 1 for n_calls, _ in per_emit), per_emit
    assert any(n_out >= 2 and n_calls == 1 for n_calls, n_out in per_emit), "no step emitted fragments of two requests"
    assert any(c is not None and any(x is None for x in c) and any(x is not None for x in c) for c in calls), \
        "no call held fragments with and without loudness"
    assert reports and all(all(len(r) >= 1 for r in rs) for rs in reports)


def test_wire_handler_takes_the_key(v2):
    req = dict(_v2_req(), media_type="raw", split_bucket=False)
    sr, a = _one(v2, dict(req, loudness=TARGET))
    sr, q = _one(v2, req)
    code, mt, body = wire.tts_handle(v2, dict(req, loudness=TARGET))
    assert code == 200 and body == a.tobytes() and body != q.tobytes()
