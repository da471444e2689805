"""GPU: the device front-end of a voice enrolment (TTS._load_refs_device, make_voices(device_frontend=True),
run_batch(device_frontend=True)) on the v2 synthetic TTS of test_voice_enrol_pipeline_gpu.py.

Files: 3.0 s at 24 kHz mono, 3.4 s at 32 kHz STEREO, 4.0 s at 16 kHz mono (its prompt is a device copy), 3.2 s at 44.1 kHz mono,
and 3.0 s of a full-scale square wave at 44.1 kHz, whose resampled peak overshoots 1 (the normalised case; load_wav reads PCM
only, so no float WAV: the normalising step is also called directly on a device stream with peaks 1.7 and 2.6).

Bars.  A resampled waveform against the host resampler's (scipy in fp64, rounded to fp32), per sample: the bar of
tests/test_resample_op_gpu.py, (t + 2) 2^-24 S + 2^-24 |ref|, with S and t from the fp64 mirror of tests/_resample_ref.py on the
file's own samples, plus 2^-24 |ref| for the host's own rounding to fp32; where the audio is normalised, 4 * 2^-24 |value| on top
(torch may multiply by a reciprocal where the kernel divides).  A spectrogram against _get_ref_spec's: twice spectrogram_torch's
error against the fp64 mirror (tests/test_spectrogram_segments_gpu.py) plus what the waveform's bar moves an fp64 spectrogram,
which is at most 1024 (the Hann window's sum) times the waveform's largest bar; fp16 rounding (2^-11 relative on each side) on top
since both sides are cast to half."""
import copy
import wave

import numpy as np
import pytest
import torch

from _resample_ref import error_bar, resample_mirror, up_down

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TEXT_A, TEXT_B = "HH AH0 L OW1 W ER1 L D .", "DH IH1 S IH1 Z AH0 T EH1 S T ."
U = 2.0 ** -24


def _write_wav(path, x, sr):
    """x [n] or [n, channels] in [-1, 1]"""
    x = np.asarray(x)
    with wave.open(path, "wb") as f:
        f.setnchannels(1 if x.ndim == 1 else x.shape[1]); f.setsampwidth(2); f.setframerate(sr)
        f.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from gsv import synthetic as S
    from gsv.text import cleaner, g2p
    from gsv.TTS_infer_pack.TTS import TTS
    cleaner.register_g2p("en", g2p.SymbolG2P())
    d = tmp_path_factory.mktemp("device_frontend")
    files = []
    for name, sec, sr, seed in (("a", 3.0, 24000, 3), ("b", 3.4, 32000, 4), ("c", 4.0, 16000, 5), ("d", 3.2, 44100, 6)):
        p = str(d / f"{name}.wav")
        x = S.make_waveform(int(sec * sr), seed, sr=sr).numpy()
        if name == "b":
            x = np.stack([x, 0.5 * S.make_waveform(int(sec * sr), 40, sr=sr).numpy()], 1)
        _write_wav(p, x, sr)
        files.append(p)
    loud = str(d / "loud.wav")
    t = np.arange(int(3.0 * 44100)) / 44100.0
    _write_wav(loud, np.sign(np.sin(2 * np.pi * 173.0 * t)), 44100)
    files.append(loud)
    short = str(d / "short.wav")
    _write_wav(short, S.make_waveform(2 * 24000, 6, sr=24000).numpy(), 24000)
    states = dict(t2s=S.make_t2s_state_dict(S.T2S_V2_CONFIG, seed=0, suppress_eos=True), vits=S.make_vits_state_dict(S.VITS_V2_CONFIG, seed=0),
                  hubert=S.make_hubert_state_dict(seed=0))

    def engine():
        tts = TTS({"device": DEV, "is_half": True, "version": "v2", "max_batch": 8, "max_seq": 600})
        tts.init_t2s_weights(state={"weight": states["t2s"], "config": S.T2S_V2_CONFIG})
        tts.init_vits_weights(state={"weight": states["vits"], "config": dict(S.VITS_V2_CONFIG)})
        tts.init_cnhuhbert_weights(state_dict=states["hubert"])
        tts.configs.max_sec = 0.4
        return tts

    specs = [dict(ref_audio_path=files[0], prompt_text=TEXT_A, prompt_lang="en"),
             dict(ref_audio_path=files[1], prompt_text=TEXT_B, prompt_lang="en"),
             dict(ref_audio_path=files[2], prompt_text=TEXT_A, prompt_lang="en"),
             dict(ref_audio_path=files[3], prompt_text=TEXT_B, prompt_lang="en"),
             dict(ref_audio_path=files[4], prompt_text=TEXT_A, prompt_lang="en")]
    return dict(dev=engine(), host=engine(), specs=specs, files=files, short=short, missing=str(d / "missing.wav"), states=states, bars={})


def _fresh(tts):
    tts.__dict__.pop("_voice_lru", None)
    return tts


def _passes(tts):
    return tts.cnhuhbert_model.model.passes


def _wave_bar(mono, sr_in, sr_out, ref):
    """the per-sample bar of a device-resampled waveform against the host's fp32 result `ref`"""
    from gsv.audio_io import resample_filter
    if sr_in == sr_out:
        return np.zeros(ref.shape[0])
    h, up, down = resample_filter(sr_in, sr_out)
    assert (up, down) == up_down(sr_in, sr_out)
    _, S, taps = resample_mirror(mono, h, up, down)
    return error_bar(ref.astype(np.float64), S, taps) + U * np.abs(ref)


def _spec64(x, n_fft=2048, hop=640):
    pad = (n_fft - hop) // 2
    xp = np.pad(np.asarray(x, dtype=np.float64), (pad, pad), mode="reflect")
    T = (xp.shape[0] - n_fft) // hop + 1
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    f = np.fft.rfft(np.stack([xp[t * hop:t * hop + n_fft] * w for t in range(T)]), axis=1)
    return np.sqrt(f.real ** 2 + f.imag ** 2 + 1e-8).T


def test_load_refs_device_against_the_host_path(world):
    from gsv.audio_io import load_wav, resample
    from gsv.module.mel_processing import spectrogram_torch
    tts, host = world["dev"], world["host"]
    cfg = tts.configs
    assert cfg.sampling_rate == 32000 and (cfg.filter_length, cfg.hop_length, cfg.win_length) == (2048, 640, 2048)
    c0 = tts.device_frontend_calls
    refs = tts._load_refs_device(world["files"] + [world["files"][1]])
    torch.cuda.synchronize()
    assert tts.device_frontend_calls == c0 + 1 and list(refs) == world["files"]              # the duplicate is read once
    tail = int(cfg.sampling_rate * 0.3)
    normalised = 0
    for path in world["files"]:
        r = refs[path]
        raw, sr = load_wav(path)
        assert r["raw_sr"] == sr and np.array_equal(r["raw_audio"], raw) and r["audio16k"] is None
        # the prompt: _prompt_wav16k's layout, the silence exactly zero
        want = host._prompt_wav16k(path)
        got = r["wav16k"].cpu().numpy()
        assert r["wav16k"].device.type == "cuda" and got.dtype == np.float32 and got.shape == want.shape
        assert np.all(got[-tail:] == 0.0) and np.all(want[-tail:] == 0.0)
        bar = _wave_bar(raw.mean(0), sr, 16000, want[:-tail])
        err = np.abs(got[:-tail].astype(np.float64) - want[:-tail])
        print(f"[device front-end] {path[-8:]}: wav16k worst err / bar {float((err / np.maximum(bar, 1e-300)).max()) if sr != 16000 else 0.0:.3f}")
        assert np.all(err <= bar)
        if sr == 16000:
            assert np.array_equal(got, want)                                                  # a device copy
        # the model-rate audio, normalised where its peak exceeds 1
        mono = raw.mean(0) if raw.shape[0] == 2 else raw[0]
        a_host = resample(mono[None], sr, cfg.sampling_rate)[0]
        bar = _wave_bar(mono, sr, cfg.sampling_rate, a_host)
        peak = float(np.abs(a_host).max())
        if peak > 1:
            normalised += 1
            div = min(2.0, peak)
            a_host = (torch.from_numpy(a_host) / div).numpy()
            bar = bar / div + 4 * U * np.abs(a_host)
        got = r["audio"].cpu().numpy()
        assert got.shape == (1, a_host.shape[0])
        err = np.abs(got[0].astype(np.float64) - a_host)
        assert np.all(err <= bar), f"{path}: audio err / bar {float((err / np.maximum(bar, 1e-300)).max())}"
        # the spectrogram: _get_ref_spec's shape and dtype, within the spectrogram bars
        spec_h, a16 = host._get_ref_spec(path)
        assert a16 is None and r["spec"].dtype == spec_h.dtype == torch.float16 and r["spec"].shape == spec_h.shape
        ref64 = _spec64(a_host)
        x32 = torch.from_numpy(a_host.astype(np.float32)).unsqueeze(0).to(DEV)
        own = np.abs(spectrogram_torch(x32, 2048, 32000, 640, 2048)[0].cpu().numpy().astype(np.float64) - ref64).max()
        moved = 1024.0 * bar.max()                    # a bin moves by at most sum_n w[n] |dx[n]|, and the Hann window sums to n_fft / 2
        sbar = (2 * own + moved) * (1 + 2.0 ** -10) + 2.0 ** -10 * ref64
        d = (r["spec"][0].float() - spec_h[0].float()).abs().cpu().numpy()
        print(f"[device front-end] {path[-8:]}: spec max abs {d.max():.3e}, worst err / bar {(d / sbar).max():.3f} "
              f"(spectrogram_torch's own {own:.3e}, waveform {moved:.3e})")
        assert np.all(d <= sbar)
    assert normalised == 1, "the square-wave file is the one whose resampled peak exceeds 1"


def test_normalising_step_on_a_device_stream(world):
    tts = world["dev"]
    g = torch.Generator().manual_seed(1)
    lens = [5, 1000, 37, 2048]
    x = torch.rand(sum(lens), generator=g) * 2 - 1
    scale = [0.9, 1.7, 1.0, 2.6]
    o = 0
    for n, s in zip(lens, scale):
        x[o:o + n] *= s / x[o:o + n].abs().max()
        o += n
    peaks = torch.tensor(scale)
    got = tts._normalise_refs(x.to(DEV), lens, peaks.to(DEV)).cpu()
    o = 0
    for n, s in zip(lens, scale):
        seg = x[o:o + n]
        want = seg / min(2.0, s) if s > 1 else seg
        if s > 1:
            assert torch.all((got[o:o + n] - want).abs() <= 4 * U * want.abs())
        else:
            assert torch.equal(got[o:o + n], want)                                           # bits unchanged
        o += n
    assert abs(got[lens[0]:lens[0] + lens[1]].abs().max().item() - 1.0) < 1e-6 and abs(got[-lens[3]:].abs().max().item() - 1.3) < 1e-6


def test_make_voices_device_frontend(world):
    tts, host, specs = _fresh(world["dev"]), _fresh(world["host"]), world["specs"]
    model = tts.cnhuhbert_model.model
    p0, c0 = _passes(tts), tts.device_frontend_calls
    seen = {}
    inner = tts._load_refs_device

    def spy(paths, **kw):
        seen["paths"] = list(paths)
        seen["refs"] = inner(paths, **kw)
        return seen["refs"]

    tts._load_refs_device = spy
    try:
        voices = tts.make_voices(specs, device_frontend=True)
    finally:
        del tts._load_refs_device
    assert _passes(tts) == p0 + 1 and model.last_pass_audios == len(specs) and tts.device_frontend_calls == c0 + 1
    assert seen["paths"] == [sp["ref_audio_path"] for sp in specs]
    # the codes: the existing code on the DOWNLOADED device prompts -- the same waveform bits give the same codes
    wavs = [seen["refs"][sp["ref_audio_path"]]["wav16k"].cpu() for sp in specs]
    feats = model.batch(wavs)
    codes = tts.vits_model.extract_latent_many([f.transpose(1, 2) for f in feats])
    refs = [host.make_voice(**sp) for sp in specs]
    for sp, v, c, r in zip(specs, voices, codes, refs):
        assert set(v) == set(r) == set(tts._VOICE_KEYS)
        assert torch.equal(v["prompt_semantic"], c[0, 0].to(DEV)) and v["prompt_semantic"].shape == r["prompt_semantic"].shape
        assert len(v["refer_spec"]) == 1 and v["refer_spec"][0][1] is None
        assert torch.equal(v["refer_spec"][0][0], seen["refs"][sp["ref_audio_path"]]["spec"])
        assert v["refer_spec"][0][0].shape == r["refer_spec"][0][0].shape and v["refer_spec"][0][0].dtype == r["refer_spec"][0][0].dtype
        assert v["phones"] == r["phones"] and v["norm_text"] == r["norm_text"] and torch.equal(v["bert_features"], r["bert_features"])
        assert v["ref_audio_path"] == sp["ref_audio_path"] and v["prompt_text"] == r["prompt_text"]
    # LRU, order and the caller's prompt cache are make_voices'
    p1, c1 = _passes(tts), tts.device_frontend_calls
    again = tts.make_voices(specs[::-1], device_frontend=True)
    assert _passes(tts) == p1 and tts.device_frontend_calls == c1 and all(x is y for x, y in zip(again, voices[::-1]))
    assert tts.prompt_cache["ref_audio_path"] is None


def test_aux_duplicates_and_errors(world):
    tts, specs, files = _fresh(world["dev"]), world["specs"], world["files"]
    p0, c0 = _passes(tts), tts.device_frontend_calls
    seen = []
    inner = tts._load_refs_device

    def spy(paths, **kw):
        seen.append((list(paths), kw))
        return inner(paths, **kw)

    tts._load_refs_device = spy
    try:
        dup = [dict(specs[0], aux_ref_audio_paths=[files[3], world["missing"]]), specs[1], dict(specs[0], prompt_text=TEXT_B), specs[1]]
        voices = tts.make_voices(dup, device_frontend=True)
    finally:
        del tts._load_refs_device
    # two distinct main references and one auxiliary (the missing one is skipped, as make_voice skips it): read once each, one call
    assert len(seen) == 1 and seen[0][0] == [files[0], files[1], files[3]] and list(seen[0][1]["prompt_paths"]) == [files[0], files[1]]
    assert _passes(tts) == p0 + 1 and tts.cnhuhbert_model.model.last_pass_audios == 2 and tts.device_frontend_calls == c0 + 1
    assert len(voices[0]["refer_spec"]) == 2 and len(voices[1]["refer_spec"]) == 1 and len(voices[2]["refer_spec"]) == 1
    assert voices[3] is voices[1] and voices[2] is not voices[0]
    assert torch.equal(voices[2]["prompt_semantic"], voices[0]["prompt_semantic"])
    # the auxiliary reference's spectrogram is the one the same file gets as a main reference
    _fresh(tts)
    main = tts.make_voices([specs[3]], device_frontend=True)[0]
    assert torch.equal(voices[0]["refer_spec"][1][0], main["refer_spec"][0][0])
    # file errors before any device work
    _fresh(tts)
    p1, c1 = _passes(tts), tts.device_frontend_calls
    with pytest.raises(OSError):
        tts.make_voices([specs[2], dict(specs[0], ref_audio_path=world["short"])], device_frontend=True)
    with pytest.raises(ValueError):
        tts.make_voices([specs[2], dict(specs[0], ref_audio_path=world["missing"])], device_frontend=True)
    with pytest.raises(ValueError):
        tts._load_refs_device([files[0], world["missing"]])
    with pytest.raises(OSError):
        tts._load_refs_device([files[0], world["short"]])
    assert _passes(tts) == p1 and tts.device_frontend_calls == c1 and not tts.__dict__.get("_voice_lru")
    # a short file is fine as an auxiliary reference (only its spectrogram is wanted), as in make_voice
    v = tts.make_voices([dict(specs[0], aux_ref_audio_paths=[world["short"]])], device_frontend=True)[0]
    assert len(v["refer_spec"]) == 2


def test_default_arguments_move_nothing(world):
    a, b, specs = _fresh(world["dev"]), _fresh(world["host"]), world["specs"]
    c0 = a.device_frontend_calls
    va, vb = a.make_voices(specs), b.make_voices(specs)
    assert a.device_frontend_calls == c0
    for x, y in zip(va, vb):
        assert torch.equal(x["prompt_semantic"], y["prompt_semantic"]) and torch.equal(x["refer_spec"][0][0], y["refer_spec"][0][0])
        assert x["phones"] == y["phones"] and torch.equal(x["bert_features"], y["bert_features"])


def test_run_batch_device_frontend(world):
    from gsv import synthetic as S
    tts, host, specs = _fresh(world["dev"]), _fresh(world["host"]), world["specs"][:4]
    utt = S.make_utterances(2)
    segs = [{"phones": it["phones"], "bert_features": torch.zeros(1024, len(it["phones"])), "norm_text": it["norm_text"]}
            for it in utt["items"]]
    reqs = [dict(sp, segments=segs, batch_size=2, top_k=1, seed=7 + i, fragment_interval=0.01) for i, sp in enumerate(specs)]
    keep = [dict(r) for r in reqs]
    with pytest.raises(ValueError, match="device_frontend"):
        tts.run_batch([dict(r) for r in reqs], device_frontend=True)
    p0, c0 = _passes(tts), tts.device_frontend_calls
    out = tts.run_batch(reqs, shared_hubert=True, device_frontend=True)
    assert _passes(tts) == p0 + 1 and tts.device_frontend_calls == c0 + 1
    assert all(a.keys() == b.keys() and "voice" not in a for a, b in zip(reqs, keep))            # requests are not mutated
    h0 = host.device_frontend_calls
    ref = host.run_batch([dict(r) for r in reqs], shared_hubert=True)
    assert host.device_frontend_calls == h0
    assert len(out) == len(ref) == len(specs)
    for (sr_a, a), (sr_b, b) in zip(out, ref):
        assert sr_a == sr_b == 32000 and a.dtype == b.dtype == np.int16 and a.shape == b.shape and np.abs(a).max() > 0
        print(f"[device front-end] run_batch: max abs int16 difference {int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max())} "
              f"(reported, not asserted: the spectrogram differs by rounding)")


def test_v2pro_shared_sv(world, tmp_path):
    """v2Pro: audio16k within the resampler's bar of the host's, then ONE compute_embedding3_many for the main and auxiliary refs"""
    from gsv import synthetic as S
    from gsv.audio_io import load_wav, resample
    from gsv.TTS_infer_pack.TTS import TTS
    pro = copy.deepcopy(S.VITS_V2_CONFIG)
    pro["model"]["version"], pro["model"]["gin_channels"] = "v2Pro", 1024
    tts = TTS({"device": DEV, "is_half": True, "version": "v2Pro", "max_batch": 4, "max_seq": 600})
    tts.init_t2s_weights(state={"weight": world["states"]["t2s"], "config": S.T2S_V2_CONFIG})
    tts.init_vits_weights(state={"weight": S.make_vits_state_dict(pro, seed=0), "config": pro})
    tts.init_cnhuhbert_weights(state_dict=world["states"]["hubert"])
    tts.init_sv_model(state_dict=S.make_eres2net_state_dict(seed=0))
    files = world["files"]
    refs = tts._load_refs_device([files[0], files[3]])
    for path in (files[0], files[3]):
        raw, sr = load_wav(path)
        a_host = resample(raw[:1], sr, 32000)
        assert float(np.abs(a_host).max()) <= 1
        want = resample(a_host, 32000, 16000)[0]
        got = refs[path]["audio16k"]
        assert got.dtype == torch.float16 and got.shape == (1, want.shape[0])
        # the device's 32 kHz audio is within its own bar of the host's; the second resampling adds its bar on the device's input
        # and carries the first one through a filter whose absolute sum bounds its gain
        from gsv.audio_io import resample_filter
        h, up, down = resample_filter(32000, 16000)
        gain = max(np.abs(h[p::up]).sum() for p in range(up))
        bar1 = _wave_bar(raw[0], sr, 32000, a_host[0]).max()
        bar = _wave_bar(a_host[0], 32000, 16000, want) + (1 + 64 * U) * gain * bar1 + 2.0 ** -11 * np.abs(want)
        assert np.all(np.abs(got[0].float().cpu().numpy().astype(np.float64) - want) <= bar)
    calls = []
    inner = tts.sv_model.compute_embedding3_many
    tts.sv_model.compute_embedding3_many = lambda wavs, **kw: (calls.append(len(wavs)), inner(wavs, **kw))[1]
    one = tts.sv_model.compute_embedding3
    tts.sv_model.compute_embedding3 = lambda *a, **k: pytest.fail("a per-reference embedding pass ran")
    try:
        specs = [dict(ref_audio_path=files[0], prompt_text=TEXT_A, prompt_lang="en", aux_ref_audio_paths=[files[3]]),
                 dict(ref_audio_path=files[1], prompt_text=TEXT_B, prompt_lang="en")]
        c0 = tts.device_frontend_calls
        voices = tts.make_voices(specs, shared_sv=True, device_frontend=True)
    finally:
        tts.sv_model.compute_embedding3_many, tts.sv_model.compute_embedding3 = inner, one
    assert calls == [3] and tts.device_frontend_calls == c0 + 1
    assert len(voices[0]["refer_spec"]) == len(voices[0]["sv_emb"]) == 2 and len(voices[1]["sv_emb"]) == 1
    assert all(e.shape == (1, 20480) and e.dtype == torch.float16 and torch.isfinite(e).all() for v in voices for e in v["sv_emb"])
    # without shared_sv the embeddings are computed per reference, as before, from the device audio16k
    _fresh(tts)
    v = tts.make_voices(specs[1:], device_frontend=True)[0]
    assert len(v["sv_emb"]) == 1 and v["sv_emb"][0].shape == (1, 20480)


def test_refused_rate_pair_goes_through_the_host_resampler(world, monkeypatch):
    """a pair the kernel refuses: that file is resampled on the host and uploaded at the target rate -- the host path's bits"""
    from gsv import audio_io as A
    from gsv.audio_io import load_wav, resample
    tts, host, files = world["dev"], world["host"], world["files"]
    monkeypatch.setattr(A, "device_resample_supported", lambda a, b: (a, b) not in [(24000, 16000), (44100, 32000)])
    refs = tts._load_refs_device(files[:4])
    for path in files[:4]:
        raw, sr = load_wav(path)
        want16 = host._prompt_wav16k(path)
        got16 = refs[path]["wav16k"].cpu().numpy()
        assert got16.shape == want16.shape
        mono = raw.mean(0) if raw.shape[0] == 2 else raw[0]
        a_host = resample(mono[None], sr, 32000)
        if sr == 24000:
            assert np.array_equal(got16, want16)
        if sr in (44100, 32000):
            assert np.array_equal(refs[path]["audio"].cpu().numpy(), a_host)
        if sr == 44100:                                               # its other pair still runs on the device
            assert not np.array_equal(got16, want16) and np.abs(got16 - want16).max() < 1e-5
