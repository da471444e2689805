"""GPU: the request key "timestamps" through every entry point, on the fp32 small v2 / v3 pipelines of the
loudness pipeline test.  With "phone": the audio is bit-equal to the default result, there is one record per sentence in output
order (batch_size = 2 and split_bucket on for v2), the phone counts are the segments', times never decrease, a sentence's first
phoneme starts at the sentence's offset and the last sentence's end + gap is len(audio) / sr to 1e-9; the same at speed_factor
1.25 and with sample_rate = 8000, encoding = "mulaw"; segments that bring word2ph get "units".  "sentence" issues no alignment
launch.  Fragments carry offsets that sum to the stream so far.  run_batch (plain, shared_sovits, shared_speed; v3 shared_cfm), the
Scheduler and a Server (whole utterances and streamed fragments) return run()'s marks per request: times within one frame (20 ms),
and every path, scored under the fp64 log-probabilities of the operands run()'s own decode of that sentence had, within 2 nf bar
of their optimum (the criterion of test_vits_align_gpu.py).  wire.tts_handle answers JSON whose base64 audio is the plain call's
bytes, also through a server; streaming_mode with the key is a 400.  inference_cli --timestamps writes the marks.  A sharded run
refuses the key; a request a server cannot plan fails alone."""
import contextlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _align_ref as R
from gsv import sharding, wire
from gsv.serving import Scheduler
from test_cli_gpu import ROOT, assets      # noqa: F401 -- the fixture with the synthetic checkpoint files
from test_output_format_pipeline_gpu import _one, _v3_req
from test_run_batch_gpu import _build, _segs, _voice_args
from test_run_batch_shared_gpu import BASE

pytestmark = pytest.mark.gpu


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


def _check(tts, req, marks, n_audio, sr_out, phone=True):
    segs = req["segments"]
    gap_s = int(tts.configs.sampling_rate * max(req.get("fragment_interval", 0.3), 0.01)) / tts._output_sr()
    assert len(marks) == len(segs) and sorted(m["index"] for m in marks) == list(range(len(segs)))
    t = 0.0
    for m in marks:
        s = segs[m["index"]]
        assert m["text"] == s["norm_text"] and abs(m["start"] - t) <= 1e-9 and m["end"] >= m["start"]
        if phone:
            assert [p[0] for p in m["phones"]] == list(s["phones"]), "the segment's phones, in order"
            assert m["phones"][0][1] == m["start"], "the first phoneme starts at the sentence's offset"
            flat = [x for p in m["phones"] for x in p[1:]]
            assert all(b >= a for a, b in zip(flat, flat[1:])) and abs(flat[-1] - m["end"]) <= 1e-9, "times never decrease"
            assert m["confidence"] is not None and m["confidence"] <= 1e-4
        else:
            assert m["phones"] == [] and m["confidence"] is None
        t = m["end"] + gap_s
    assert abs(t - n_audio / sr_out) <= 1e-9, (t, n_audio / sr_out)


@contextlib.contextmanager
def _operands_of_run(tts):
    """while run() decodes with alignment spans: per span, the fp64 log-probabilities (tests/_align_ref.py) of the MRTE attention's
    own operands of that decode, their bar, the frames and the ends the engine found -> list of dicts, in decode order"""
    m, caps, held = tts.vits_model, [], []
    begin, end = m._align_begin, m._align_end

    def spy_begin(spans):
        held.append(list(spans))
        return begin(spans)

    def spy_end(pend):
        end(pend)
        if pend is None:
            return
        q = m.debug_tensor("m_q", 512 * 4096).view(512, -1).t().double().cpu().numpy()
        k = m.debug_tensor("m_kv", 1024 * 2048).view(1024, -1).t()[:, :512].double().cpu().numpy()
        for (seg, c0, nc, p0, npn), (ends, score) in zip(held.pop(), m.last_alignment):
            assert seg == 0
            lp, a_max, s_max = R.logp_mirror(q[2 * c0:2 * (c0 + nc)], k[p0:p0 + npn], 4, 128 ** -0.5)
            caps.append(dict(nl=npn, nf=2 * nc, lp=lp, bar=float(R.logp_bar(lp, a_max, s_max, 4, 128, 128 ** -0.5).max()),
                             ends=np.asarray(ends)))
    m._align_begin, m._align_end = spy_begin, spy_end
    try:
        yield caps
    finally:
        del m._align_begin, m._align_end


def _ends_of(mark, nf):
    """the integer ends a record's phoneme times stand for"""
    dur = mark["end"] - mark["start"]
    return np.array([int(round((p[2] - mark["start"]) / dur * nf)) for p in mark["phones"]], np.int64)


def _same_marks(got, ref, caps, what):
    """`got` against run()'s `ref`: the same sentences and phones, times within one 20 ms frame, and every searched path within
    2 nf bar of the optimum under the operands of run()'s decode of that sentence (caps, matched by phone count and ends)"""
    assert [m["index"] for m in got] == [m["index"] for m in ref]
    for a, b in zip(got, ref):
        assert abs(a["start"] - b["start"]) <= 0.02 and abs(a["end"] - b["end"]) <= 0.02
        assert [p[0] for p in a["phones"]] == [p[0] for p in b["phones"]]
        assert all(abs(x[1] - y[1]) <= 0.02 and abs(x[2] - y[2]) <= 0.02 for x, y in zip(a["phones"], b["phones"])), what
        if not a["phones"]:
            continue
        fits = [c for c in caps if c["nl"] == len(b["phones"]) and _ends_of(b, c["nf"]).tolist() == c["ends"].tolist()]
        assert fits, "run()'s times are the ends its engine found for the sentence"
        cap = fits[0]
        nf, nl = cap["lp"].shape
        if not R.searched(nf, nl):
            assert _ends_of(a, nf).tolist() == R.fallback_ends(nf, nl).tolist() and a["confidence"] == -np.inf
            continue
        _, _, V = R.dp_mirror(cap["lp"], keep64=True)
        loss = V[nl - 1] - R.path_sum(cap["lp"], _ends_of(a, nf))
        print(f"[timestamps] {what}: nf {nf} nl {nl} loss {loss:.3e} of 2 nf bar {2 * nf * cap['bar']:.3e}")
        assert loss <= 2 * nf * cap["bar"], (what, loss)


def _run_marks(tts, req):
    """run()'s (sr, audio, marks) of the request with the current prompt cache, and the operands of its decodes"""
    with _operands_of_run(tts) as caps:
        out = _one(tts, {k: v for k, v in req.items() if k != "voice"})
    return out, caps


@pytest.mark.parametrize("model", ["v2", "v3"])
def test_run_with_phone_marks(model, request):
    tts = request.getfixturevalue(model)
    req = _v2_req() if model == "v2" else _v3_req()
    sr, q = _one(tts, req)
    assert tts.last_timestamps == []
    out = _one(tts, dict(req, timestamps="phone"))
    assert len(out) == 3 and out[0] == sr and np.array_equal(out[1], q), "the audio does not depend on the key"
    marks = out[2]
    assert marks is tts.last_timestamps
    if model == "v2":
        assert [m["index"] for m in marks] == [0, 1, 2], "buckets are put back in submission order"
    _check(tts, req, marks, len(q), sr)
    assert all("units" not in m for m in marks)
    assert _one(tts, req)[1].tobytes() == q.tobytes() and tts.last_timestamps == [], "replaced, never extended"
    if model == "v2":       # segments that bring word2ph (the zh pre-processor's key): characters with their times
        segs = [dict(sg, word2ph=[len(sg["phones"]) - len(sg["norm_text"]) + 1] + [1] * (len(sg["norm_text"]) - 1))
                for sg in req["segments"]]
        sr2, a, units = _one(tts, dict(req, segments=segs, timestamps="phone"))
        assert np.array_equal(a, q) and [m["phones"] for m in units] == [m["phones"] for m in marks]
        for m in units:
            sg = segs[m["index"]]
            assert [u[0] for u in m["units"]] == list(sg["norm_text"]) and m["units"][0][1] == m["start"]
            assert m["units"][0][2] == m["phones"][sg["word2ph"][0] - 1][2] and abs(m["units"][-1][2] - m["end"]) <= 1e-9


def test_run_at_another_speed_and_in_another_format(v2):
    req = dict(_v2_req(), speed_factor=1.25)
    sr, q = _one(v2, req)
    sr2, a, marks = _one(v2, dict(req, timestamps="phone"))
    assert np.array_equal(a, q)
    _check(v2, req, marks, len(q), sr)
    req = dict(_v2_req(), sample_rate=8000, encoding="mulaw")
    sr, q = _one(v2, req)
    sr2, a, marks2 = _one(v2, dict(req, timestamps="phone"))
    assert sr == sr2 == 8000 and a.dtype == np.uint8 and np.array_equal(a, q)
    _check(v2, req, marks2, len(q), 8000)
    plain = _one(v2, dict(_v2_req(), timestamps="phone"))[2]
    assert [m["phones"] for m in marks2] == [m["phones"] for m in plain], "seconds: the output format does not move them"


def test_sentence_marks_issue_no_alignment(v2):
    req = _v2_req()
    sr, q = _one(v2, req)
    v2.vits_model.last_alignment = None
    # the engine issues its two alignment launches iff a span table is pending (gsv_vits_set_align), and the one place that makes
    # one pending is _align_begin: counting its calls counts the launches the key adds to a decode
    calls, begin = [], v2.vits_model._align_begin
    v2.vits_model._align_begin = lambda spans: calls.append(len(spans)) or begin(spans)
    try:
        sr2, a, marks = _one(v2, dict(req, timestamps="sentence"))
        assert calls == [], "no table pending: every decode issues the launches it issues without the key"
        assert np.array_equal(a, q) and v2.vits_model.last_alignment is None
        _one(v2, dict(req, timestamps="phone"))
        assert calls and sum(calls) == 3, "one table per waveform pass, one span per sentence of its fold"
    finally:
        del v2.vits_model._align_begin
    _check(v2, req, marks, len(q), sr, phone=False)
    phone = _one(v2, dict(req, timestamps="phone"))[2]
    assert [(m["start"], m["end"]) for m in marks] == [(m["start"], m["end"]) for m in phone]
    with pytest.raises(ValueError):
        list(v2.run(dict(req, timestamps="word")))


def test_fragments_carry_their_offset_in_the_stream(v2):
    req = dict(_v2_req(), return_fragment=True)
    plain = list(v2.run(dict(req)))
    out = list(v2.run(dict(req, timestamps="phone")))
    assert len(out) == len(plain) == 2 and all(len(f) == 3 for f in out)
    t = 0.0
    for (sr, q), (sr2, a, marks) in zip(plain, out):
        assert np.array_equal(a, q) and marks and all(abs(m["offset"] - t) <= 1e-9 for m in marks)
        assert marks[0]["start"] == 0.0, "times are relative to the fragment"
        gap_s = int(v2.configs.sampling_rate * 0.01) / sr
        assert abs(marks[-1]["end"] + gap_s - len(q) / sr) <= 1e-9
        t += len(q) / sr
    assert sorted(m["index"] for f in out for m in f[2]) == [0, 1, 2]


def test_wire_answers_json_with_the_audio_as_base64(v2):
    import base64
    import json
    req = dict(_v2_req(), media_type="raw")
    code, mt, plain = wire.tts_handle(v2, dict(req))
    assert code == 200 and mt == "audio/raw"
    code, mt, payload = wire.tts_handle(v2, dict(req, timestamps="phone"))
    assert code == 200 and mt == "application/json"
    payload = json.loads(json.dumps(payload))                                    # it is JSON as it stands
    assert base64.b64decode(payload["audio"]) == plain, "the packed media of the plain call, byte for byte"
    assert payload["media_type"] == "raw" and payload["sample_rate"] == 32000
    marks = payload["timestamps"]
    assert [m["index"] for m in marks] == [0, 1, 2]
    assert [[p[0] for p in m["phones"]] for m in marks] == [list(s["phones"]) for s in req["segments"]]
    assert abs(marks[-1]["end"] + int(32000 * 0.01) / 32000 - len(plain) / 2 / 32000) <= 1e-9
    # streaming_mode with timestamps is refused before any stage runs, and the query-string form of the key is parsed
    code, mt, payload = wire.tts_handle(v2, dict(req, timestamps="phone", streaming_mode=True))
    assert code == 400 and "timestamps" in payload["Exception"]
    assert wire.parse_timestamps("false") is False and wire.parse_timestamps("0") is False
    assert wire.parse_timestamps("Phone") == "phone" and wire.parse_timestamps("sentence") == "sentence"
    assert wire.tts_handle(v2, dict(req, timestamps=wire.parse_timestamps("false")))[1] == "audio/raw"


@pytest.mark.parametrize("kw", [{}, {"shared_sovits": True}, {"shared_sovits": True, "shared_speed": True}],
                         ids=["plain", "shared_sovits", "shared_speed"])
def test_run_batch_returns_the_marks_of_run(v2, kw):
    kws = [_voice_args(0, 8, 6, "v2"), _voice_args(1, 23, 4, "v2")]
    voices = [v2.make_voice(**k) for k in kws]
    reqs = [dict(BASE, segments=_segs(61, [9, 5, 7]), batch_size=2, seed=3, voice=voices[0], timestamps="phone"),
            dict(BASE, segments=_segs(62, [7, 12]), batch_size=2, seed=4, voice=voices[1], speed_factor=1.25, timestamps="phone"),
            dict(BASE, segments=_segs(63, [6, 8]), batch_size=2, seed=5, voice=voices[0], timestamps="sentence"),
            dict(BASE, segments=_segs(64, [5]), batch_size=2, seed=6, voice=voices[1])]
    plain = v2.run_batch([{k: v for k, v in r.items() if k != "timestamps"} for r in reqs], **kw)
    assert v2.last_timestamps == [[], [], [], []]
    got = v2.run_batch([dict(r) for r in reqs], **kw)
    assert [len(g) for g in got] == [3, 3, 3, 2]
    assert all(g[0] == p[0] and np.array_equal(g[1], p[1]) for g, p in zip(got, plain)), "the audio does not depend on the key"
    assert v2.last_timestamps == [got[0][2], got[1][2], got[2][2], []]
    try:
        for n, (r, kwv, g) in enumerate(zip(reqs[:3], [kws[0], kws[1], kws[0]], got)):
            v2.set_prompt_cache(**kwv)
            (sr, audio, marks), caps = _run_marks(v2, r)
            _check(v2, r, g[2], len(g[1]), g[0], phone=r["timestamps"] == "phone")
            _same_marks(g[2], marks, caps, f"run_batch {kw} request {n}")
    finally:
        v2.set_prompt_cache(**_voice_args(0, 8, 6, "v2"))


def test_run_batch_shared_cfm_returns_the_marks_of_run(v3):
    req = dict(_v3_req(), timestamps="phone")
    plain = v3.run_batch([_v3_req()], shared_cfm=True)[0]
    got = v3.run_batch([dict(req)], shared_cfm=True)[0]
    assert len(got) == 3 and got[0] == plain[0] and np.array_equal(got[1], plain[1])
    (sr, audio, marks), caps = _run_marks(v3, req)
    _check(v3, req, got[2], len(got[1]), got[0])
    _same_marks(got[2], marks, caps, "run_batch shared_cfm")


def _requests(v2):
    kws = [_voice_args(0, 8, 6, "v2"), _voice_args(1, 23, 4, "v2")]
    voices = [v2.make_voice(**k) for k in kws]
    reqs = [dict(BASE, segments=_segs(61, [9, 5, 7]), batch_size=2, seed=3, voice=voices[0], timestamps="phone"),
            dict(BASE, segments=_segs(62, [7, 12]), batch_size=2, seed=4, voice=voices[1], speed_factor=1.25, timestamps="phone"),
            dict(BASE, segments=_segs(63, [6, 8]), batch_size=2, seed=5, voice=voices[0], timestamps="sentence"),
            dict(BASE, segments=_segs(64, [5]), batch_size=2, seed=6, voice=voices[1])]
    return reqs, [kws[0], kws[1], kws[0], kws[1]]


def test_the_scheduler_returns_the_marks_of_run(v2):
    reqs, kws = _requests(v2)
    results = {}
    with Scheduler(v2, slots=4, chunk=32) as sch:
        tickets = [sch.submit(dict(r)) for r in reqs]
        for _ in range(400):
            results.update(sch.step())
            if sch.idle:
                break
        assert sch.idle
    got = [results[t] for t in tickets]
    assert not any(isinstance(g, BaseException) for g in got), got
    assert [len(g) for g in got] == [3, 3, 3, 2]
    try:
        for n, (r, kwv, g) in enumerate(zip(reqs[:3], kws, got)):
            v2.set_prompt_cache(**kwv)
            (sr, audio, marks), caps = _run_marks(v2, r)
            assert g[0] == sr and g[1].shape == audio.shape
            _check(v2, r, g[2], len(g[1]), g[0], phone=r["timestamps"] == "phone")
            _same_marks(g[2], marks, caps, f"scheduler request {n}")
    finally:
        v2.set_prompt_cache(**_voice_args(0, 8, 6, "v2"))


def test_a_server_streams_fragments_with_offsets_and_answers_the_wire(v2):
    reqs, kws = _requests(v2)
    try:
        v2.set_prompt_cache(**kws[0])
        with _operands_of_run(v2) as caps:
            ref = list(v2.run({k: v for k, v in dict(reqs[0], return_fragment=True).items() if k != "voice"}))
        (sr1, a1, m1), caps1 = _run_marks(v2, reqs[0])
    finally:
        v2.set_prompt_cache(**_voice_args(0, 8, 6, "v2"))
    server = v2.serve(slots=4, chunk=4)
    try:
        frags = list(server.submit_stream(dict(reqs[0])))
        whole = server.submit(dict(reqs[0])).result(timeout=120)
        code, mt, payload = wire.tts_handle(v2, dict(reqs[0], media_type="raw"), server=server)
        bad = server.submit(dict(reqs[0], timestamps="word"))
        with pytest.raises(ValueError, match="timestamps"):
            bad.result(timeout=120)
        plain = server.submit({k: v for k, v in reqs[0].items() if k != "timestamps"}).result(timeout=120)
        assert server.error is None, "a request that cannot be planned fails alone"
    finally:
        server.shutdown(timeout=120)
    assert len(frags) == len(ref) == 2 and all(len(f) == 3 for f in frags)
    t = 0.0
    for (sr, a, marks), (sr_r, a_r, marks_r) in zip(frags, ref):
        assert sr == sr_r and a.shape == a_r.shape
        assert marks and all(abs(m["offset"] - t) <= 1e-9 for m in marks), "offsets sum to the stream so far"
        assert marks[0]["start"] == 0.0 and abs(marks[-1]["end"] + int(32000 * 0.01) / sr - len(a) / sr) <= 1e-9
        _same_marks(marks, marks_r, caps, "streamed fragment")
        t += len(a) / sr
    assert len(whole) == 3 and len(plain) == 2 and whole[1].shape == plain[1].shape
    _same_marks(whole[2], m1, caps1, "server, whole utterance")
    assert code == 200 and mt == "application/json"
    payload = json.loads(json.dumps(payload))
    assert len(payload["timestamps"]) == 3 and len(payload["audio"]) > 0 and payload["sample_rate"] == 32000


def test_inference_cli_writes_the_marks(assets):       # noqa: F811
    d = assets
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "gpt-sovits_amd") + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = d / "marks.json"
    cmd = [sys.executable, "-m", "gsv.inference_cli", "--gpt_model", str(d / "gpt.ckpt"), "--sovits_model", str(d / "sovits.pth"),
           "--ref_audio", str(d / "ref.wav"), "--ref_text", str(d / "ref.txt"), "--ref_language", "英文",
           "--target_text", str(d / "target.txt"), "--target_language", "英文", "--output_path", str(d / "out_ts"),
           "--cnhubert_base_path", str(d / "hubert"), "--frontend", "symbols", "--timestamps", str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Timestamps saved to" in r.stdout
    marks = json.loads(out.read_text(encoding="utf-8"))
    assert len(marks) == 1 and marks[0]["start"] == 0.0 and abs(marks[0]["end"] - 30 * 1280 / 32000) <= 1e-9
    ph = marks[0]["phones"]
    assert len(ph) >= 10 and ph[0][1] == 0.0 and abs(ph[-1][2] - marks[0]["end"]) <= 1e-9
    assert all(y[1] == x[2] and y[2] > y[1] for x, y in zip(ph, ph[1:])) and marks[0]["confidence"] <= 1e-4


def test_a_sharded_run_refuses_the_key(v2):
    with pytest.raises(ValueError, match="timestamps"):
        sharding.refuse_output_format([dict(_v2_req(), timestamps="phone")])
