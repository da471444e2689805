"""GPU: the request keys "sample_rate" and "encoding"  through run, run_batch, the server and its streams,
on the fp32 small v2 pipeline of test_run_batch_gpu.py and the small v3 pipeline of test_audio_sr_gpu.py.

The bar of a resampled result against the host resampler on the default result q (int16), in int16 LSB: the default path
truncates, so the waveform x has |x - q / 32768| < 2^-15 per sample; the FIR turns that into at most A LSB, A the largest
absolute sum of one polyphase branch of the filter (computed here); the output truncation adds 1 and the fp32 accumulation stays
under 1: (A + 2) LSB.  Between two runs of the same request whose waveforms are within 1 LSB (the serving bar): (A + 1) LSB."""
import numpy as np
import pytest

from gsv import _lib, audio_io
from gsv.serving import Scheduler, plan_online
from test_run_batch_gpu import DEV, _build, _segs, _voice_args
from test_run_batch_shared_gpu import BASE, _lsb
from test_serving_stream_gpu import _drive, _run_stream

pytestmark = pytest.mark.gpu
WAIT = 120.0
RATES = [8000, 16000, 44100]


def _A(sr_in, sr_out):
    h, up, down = audio_io.resample_filter(sr_in, sr_out)
    return max(float(np.abs(h[p::up].astype(np.float64)).sum()) for p in range(up))


def _host(q, sr_in, sr_out):
    """trunc(32768 * audio_io.resample(q / 32768)), saturated as the kernel saturates"""
    y = audio_io.resample(q.astype(np.float32) / np.float32(32768.0), sr_in, sr_out)
    return np.clip(np.trunc(y.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int32)


def _ulaw2lin(codes):
    """G.711 mu-law decoding -> (int32 samples, the quantisation step at each)"""
    u = ~codes.astype(np.int32) & 0xff
    seg = (u >> 4) & 7
    t = (((u & 0xf) << 3) + 0x84) << seg
    return np.where(u & 0x80, 0x84 - t, t - 0x84), 8 << seg


def test_ulaw_decoder():
    codes = np.arange(256, dtype=np.uint8)
    lin, step = _ulaw2lin(codes)
    assert lin[0xff] == 0 and lin[0x7f] == 0 and lin[0x80] == 32124 and lin[0x00] == -32124 and step[0xff] == 8 and step[0x80] == 1024
    try:
        import audioop
    except ImportError:                                                 # a Python without it: the corner values above stand
        return
    assert lin.tolist() == np.frombuffer(audioop.ulaw2lin(codes.tobytes(), 2), dtype="<i2").tolist()


def _peaks(tts, scale):
    """records max |x| of every sentence audio_postprocess is handed, after scaling it by `scale` (the small v3 vocoder's
    random weights drive its output to full scale, where the default path divides by the peak or wraps at +1.0)"""
    seen, inner = [], tts.audio_postprocess

    def spy(audio, *a, **k):
        audio = [[f * scale for f in b] for b in audio]
        seen.extend(float(f.abs().max()) for b in audio for f in b if f.numel())
        return inner(audio, *a, **k)
    tts.audio_postprocess = spy
    return seen


@pytest.fixture(scope="module")
def v2():
    tts = _build("v2")
    tts.set_prompt_cache(**_voice_args(0, 8, 6, "v2"))
    return tts


@pytest.fixture(scope="module")
def v3():
    from test_audio_sr_gpu import _tts_with_sr
    return _tts_with_sr("v3")


def _v3_req():
    from test_audio_sr_gpu import _segs as segs3
    return {"segments": segs3(), "batch_size": 3, "top_k": 1, "seed": 3, "sample_steps": 2, "fragment_interval": 0.01}


def _one(tts, req):
    out = list(tts.run(dict(req)))
    assert len(out) == 1
    return out[0]


@pytest.mark.parametrize("model", ["v2", "v3"])
def test_run_at_other_rates(model, request):
    tts = request.getfixturevalue(model)
    req = dict(BASE, segments=_segs(60, [9, 5, 7]), batch_size=2, seed=3) if model == "v2" else _v3_req()
    sr0 = 32000 if model == "v2" else 24000
    peaks = _peaks(tts, 1.0 if model == "v2" else 0.5)
    try:
        sr, q = _one(tts, req)
        assert sr == sr0 and q.dtype == np.int16 and q.size > 0 and np.abs(q).max() > 0
        assert peaks and max(peaks) < 1.0, "a sentence is normalised or wraps: q is then not the truncated waveform"
        same = _one(tts, dict(req, sample_rate=sr0, encoding="pcm_s16"))
        assert same[0] == sr0 and same[1].dtype == np.int16 and np.array_equal(same[1], q)
        for r in RATES:
            sr, a = _one(tts, dict(req, sample_rate=r))
            assert sr == r and a.dtype == np.int16 and a.shape == (audio_io.resampled_len(len(q), sr0, r),)
            bar, worst = _A(sr0, r) + 2.0, _lsb(a, _host(q, sr0, r))
            print(f"\n{model} {sr0} -> {r}: {worst} LSB from the host resampler, bar {bar:.2f}")
            assert worst <= bar
        # an encoding at the model's own rate: G.711 of the default result
        sr, codes = _one(tts, dict(req, encoding="mulaw"))
        assert sr == sr0 and codes.dtype == np.uint8 and codes.shape == q.shape
        lin, step = _ulaw2lin(codes)
        assert (np.abs(lin - q.astype(np.int32)) <= step).all()
    finally:
        del tts.audio_postprocess
    with pytest.raises(ValueError):
        tts._resolve_options(dict(req, sample_rate=44101))


def test_v3_super_sampling_then_16k(v3):
    sr48, a48 = _one(v3, dict(_v3_req(), super_sampling=True))
    sr, a = _one(v3, dict(_v3_req(), super_sampling=True, sample_rate=16000))
    assert sr48 == 48000 and sr == 16000 and a.dtype == np.int16
    assert a.shape == (audio_io.resampled_len(len(a48), 48000, 16000),) and np.abs(a).max() > 0
    same = _one(v3, dict(_v3_req(), super_sampling=True, sample_rate=48000))
    assert same[0] == 48000 and np.array_equal(same[1], a48)


FORMATS = [{}, {"sample_rate": 8000, "encoding": "mulaw"}, {"sample_rate": 44100}]


def _meets(got, want, fmt, what):
    assert not isinstance(got, BaseException), f"{what} raised {got!r}"
    (sr, a), (sr0, a0) = got, want
    assert sr == sr0 == fmt.get("sample_rate", 32000) and a.dtype == a0.dtype and a.shape == a0.shape, what
    if fmt.get("encoding") == "mulaw":
        assert a.dtype == np.uint8
        (x, sx), (y, sy) = _ulaw2lin(a), _ulaw2lin(a0)
        assert (np.abs(x - y) <= np.maximum(sx, sy)).all(), f"{what}: more than a code step apart"
    elif "sample_rate" in fmt:
        assert _lsb(a, a0) <= _A(32000, fmt["sample_rate"]) + 1.0, f"{what}: {_lsb(a, a0)} LSB"
    else:
        assert a.dtype == np.int16 and _lsb(a, a0) <= 1, f"{what}: {_lsb(a, a0)} LSB"


@pytest.fixture(scope="module")
def burst(v2):
    """three requests of three voices, one per format, each with run_batch([request]) alone"""
    kws = [_voice_args(0, 8, 6, "v2"), _voice_args(1, 23, 4, "v2"), _voice_args(2, 5, 7, "v2")]
    voices = [v2.make_voice(**kw) for kw in kws]
    reqs = [dict(BASE, segments=_segs(61 + i, lens), batch_size=2, seed=3 + i, voice=voices[i], **FORMATS[i])
            for i, lens in enumerate([[9, 5, 7], [7, 12], [11, 6, 8]])]
    alone = [v2.run_batch([dict(r)])[0] for r in reqs]
    assert [a[1].dtype for a in alone] == [np.int16, np.uint8, np.int16] and [a[0] for a in alone] == [32000, 8000, 44100]
    return kws, reqs, alone


def test_run_batch_and_server_with_mixed_formats(v2, burst):
    _, reqs, alone = burst
    out = v2.run_batch([dict(r) for r in reqs], shared_sovits=True)
    for i in range(3):
        _meets(out[i], alone[i], FORMATS[i], f"run_batch request {i}")
    server = v2.serve(slots=4, chunk=4)
    try:
        futs = [server.submit(dict(r)) for r in reqs]
        for i, f in enumerate(futs):
            _meets(f.result(timeout=WAIT), alone[i], FORMATS[i], f"server request {i}")
    finally:
        server.shutdown(timeout=WAIT)
    assert server.error is None


def test_streams_with_mixed_formats_one_launch_pair_per_format(v2, burst):
    kws, reqs, _ = burst
    fmts = [FORMATS[1], FORMATS[2], FORMATS[1], FORMATS[0]]
    batch = [dict({k: v for k, v in reqs[i % 3].items() if k not in ("sample_rate", "encoding")}, seed=20 + i, return_fragment=True,
                  **fmt) for i, fmt in enumerate(fmts)]
    want = []
    for i, req in enumerate(batch):
        plain = {k: v for k, v in req.items() if k not in ("return_fragment", "voice")}
        want.append(_run_stream(v2, kws[i % 3], plain))
    l = _lib.lib()
    inner, calls = l.gsv_postprocess_groups_rate, []

    def counted(*a):
        calls.append(int(a[-2]))                                        # out_fmt
        return inner(*a)
    per_step = []                                                       # (rate calls, the formats of the fragments emitted)
    results, plans, frag_steps = {}, {}, {}
    l.gsv_postprocess_groups_rate = counted
    try:
        with Scheduler(v2, slots=4, chunk=32) as sched:
            take = sched.take_fragments

            def taking():
                out = take()
                if out:
                    per_step.append((list(calls), [tuple(sorted(fmts[t].items())) for t, _, _ in out]))
                    calls.clear()
                return out
            sched.take_fragments = taking
            emit = sched._emit

            def emitting(due, ends):                                    # the plans, before a request that ends is dropped
                for t, pl in sched._requests.items():
                    if isinstance(pl, dict) and "stream" in pl:
                        plans.setdefault(t, pl)
                return emit(due, ends)
            sched._emit = emitting
            ticket_of = _drive(sched, batch, [[0, 1, 2, 3]], plans, results, frag_steps)
            stats = sched.stats
    finally:
        l.gsv_postprocess_groups_rate = inner
    assert [ticket_of[r] for r in range(4)] == [0, 1, 2, 3]
    for r in range(4):
        frags, toks = want[r]
        assert isinstance(results[r], list) and len(results[r]) == len(frags), f"stream {r}: {len(results[r])} fragments"
        assert [[p.cpu().tolist() for p in pred] for pred in plans[r]["preds"]] == toks
        for bi, (g, w) in enumerate(zip(results[r], frags)):
            _meets(g, w, fmts[r], f"stream {r} fragment {bi}")
    for n_calls, emitted in per_step:
        other = {f for f in emitted if f}
        assert len(n_calls) == len(other), f"{len(n_calls)} gsv_postprocess_groups_rate calls for the formats {sorted(other)}"
    assert any(len({f for f in emitted if f}) == 2 for _, emitted in per_step), "no step emitted fragments of two formats"
    idxs = {r: [[int(i) for i in idx] for idx in plans[r]["idxs"]] for r in range(4)}
    lengths = [n for r in range(4) for idx in idxs[r] for n in idx]
    plan = plan_online([stats["tickets"][t][0] for t in range(4)], [len(batch[r]["segments"]) for r in range(4)], lengths, slots=4,
                       chunk=32, streaming={r: [len(idx) for idx in idxs[r]] for r in range(4)})
    assert stats["events"] == plan
