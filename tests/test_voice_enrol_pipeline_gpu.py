"""GPU: TTS.make_voices and run_batch(shared_hubert=True): many reference voices enrolled with one packed HuBERT pass and one
extract_latent_many, against make_voice per spec.  v2 synthetic TTS as in test_set_ref_audio_end_to_end; three WAV files (3.0 s
at 24 kHz, 3.4 s at 32 kHz, 4.0 s at 16 kHz), two of them sharing one prompt text.

What is bit-equal by construction (computed per voice by the code make_voice runs): refer_spec, phones, bert_features,
norm_text.  The prompt codes come from the packed pass: they are compared where the mirror's VQ margin (squared distance to the
second-nearest code minus that to the nearest, oracle.vits_oracle.VitsOracle.extract_latent's arithmetic on
tests/_hubert_ref.py's features) is above 1.0, and such positions must be at least 90 % of all, asserted on the mirror alone.
With the synthetic VITS weights every frame quantises to the same code, so this pins the plumbing (right voice, right length);
the arithmetic of the pass is pinned by tests/test_hubert_batch_gpu.py."""
import wave

import numpy as np
import pytest
import torch

import _hubert_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TEXT_A, TEXT_B = "HH AH0 L OW1 W ER1 L D .", "DH IH1 S IH1 Z AH0 T EH1 S T ."


def _write_wav(path, x, sr):
    with wave.open(path, "wb") as f:
        f.setnchannels(1); f.setsampwidth(2); f.setframerate(sr)
        f.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from gsv import synthetic as S
    from gsv.text import cleaner, g2p
    from gsv.TTS_infer_pack.TTS import TTS
    cleaner.register_g2p("en", g2p.SymbolG2P())
    d = tmp_path_factory.mktemp("enrol")
    files = []
    for name, sec, sr, seed in (("a", 3.0, 24000, 3), ("b", 3.4, 32000, 4), ("c", 4.0, 16000, 5)):
        p = str(d / f"{name}.wav")
        _write_wav(p, S.make_waveform(int(sec * sr), seed, sr=sr).numpy(), sr)
        files.append(p)
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
             dict(ref_audio_path=files[2], prompt_text=TEXT_A, prompt_lang="en")]
    return dict(many=engine(), single=engine(), specs=specs, files=files, short=short, missing=str(d / "missing.wav"),
                states=states)


def _fresh(tts):
    """an engine that has enrolled nothing: the voice LRU is what make_voice / make_voices keep between calls"""
    tts.__dict__.pop("_voice_lru", None)
    return tts


def _passes(tts):
    return tts.cnhuhbert_model.model.passes


def _mirror_margins(world, tts, path):
    """per code position: squared distance to the second-nearest code minus that to the nearest, on the mirror's features"""
    from gsv import synthetic as S
    from oracle.vits_oracle import VitsOracle
    feat = R.hubert(world["states"]["hubert"], torch.from_numpy(tts._prompt_wav16k(path)))["last_hidden_state"]      # [T50, 768]
    o = VitsOracle(world["states"]["vits"], S.VITS_V2_CONFIG)
    x = o.conv(feat.t().float(), "ssl_proj", stride=2, padding=0).t()
    e = o.sd["quantizer.vq.layers.0._codebook.embed"].t()
    d2 = x.pow(2).sum(1, keepdim=True) - 2 * x @ e + e.pow(2).sum(0, keepdim=True)
    two = d2.topk(2, dim=-1, largest=False)
    return two.values[:, 1] - two.values[:, 0], two.indices[:, 0]


def test_make_voices_matches_make_voice(world):
    many, single, specs = _fresh(world["many"]), _fresh(world["single"]), world["specs"]
    p0 = _passes(many)
    voices = many.make_voices(specs)
    assert _passes(many) == p0 + 1 and many.cnhuhbert_model.model.last_pass_audios == 3
    s0 = _passes(single)
    refs = [single.make_voice(**sp) for sp in specs]
    assert _passes(single) == s0                                   # the per-voice path makes no packed pass
    assert len(voices) == 3
    for sp, v, r in zip(specs, voices, refs):
        assert set(v) == set(r) == set(many._VOICE_KEYS)
        assert len(v["refer_spec"]) == len(r["refer_spec"]) == 1 and torch.equal(v["refer_spec"][0][0], r["refer_spec"][0][0])
        assert v["phones"] == r["phones"] and v["norm_text"] == r["norm_text"] and len(v["phones"]) >= 6
        assert torch.equal(v["bert_features"], r["bert_features"])
        assert v["ref_audio_path"] == r["ref_audio_path"] == sp["ref_audio_path"] and v["prompt_text"] == r["prompt_text"]
        a, b = v["prompt_semantic"], r["prompt_semantic"]
        assert a.dtype == b.dtype == torch.int64 and a.shape == b.shape and a.dim() == 1
        margin, near = _mirror_margins(world, many, sp["ref_audio_path"])
        assert margin.numel() == a.numel()
        clear = margin > 1.0
        print(f"[voice enrol] {sp['ref_audio_path'][-5:]}: {a.numel()} codes, smallest mirror margin {float(margin.min()):.2f}, "
              f"clear {int(clear.sum())} / {clear.numel()}")
        assert int(clear.sum()) >= 0.9 * clear.numel()
        assert torch.equal(a.cpu()[clear], b.cpu()[clear]) and torch.equal(a.cpu()[clear], near[clear])
    # 3.0 s + 0.3 s * 32000 / 16000 of silence = 57600 samples -> 179 frames -> 89 codes; 3.4 s -> 64000 -> 99; 4.0 s -> 73600 -> 114
    assert [v["prompt_semantic"].numel() for v in voices] == [89, 99, 114]
    assert voices[0]["phones"] == voices[2]["phones"] != voices[1]["phones"]
    # a repeated call makes no pass and returns the LRU's objects
    p1 = _passes(many)
    again = many.make_voices(specs)
    assert _passes(many) == p1 and all(x is y for x, y in zip(again, voices))
    assert many.make_voice(**specs[1]) is voices[1]
    assert many.prompt_cache["ref_audio_path"] is None             # the caller's prompt cache is not touched


def test_duplicate_paths_errors_and_eviction(world):
    many, specs = _fresh(world["many"]), world["specs"]
    # two specs on one file (different prompt texts): the audio runs once
    p0 = _passes(many)
    dup = [specs[0], specs[1], dict(specs[0], prompt_text=TEXT_B), specs[0]]
    voices = many.make_voices(dup)
    assert _passes(many) == p0 + 1 and many.cnhuhbert_model.model.last_pass_audios == 2
    assert voices[3] is voices[0] and voices[2] is not voices[0]
    assert torch.equal(voices[2]["prompt_semantic"], voices[0]["prompt_semantic"]) and voices[2]["phones"] == voices[1]["phones"]
    # file errors are raised before any device work, whatever stands in front of them
    _fresh(many)
    p0 = _passes(many)
    with pytest.raises(OSError):
        many.make_voices([specs[2], dict(specs[0], ref_audio_path=world["short"])])
    with pytest.raises(ValueError):
        many.make_voices([specs[2], dict(specs[0], ref_audio_path=world["missing"])])
    with pytest.raises(ValueError):
        many.make_voices([dict(prompt_text=TEXT_A, prompt_lang="en")])
    assert _passes(many) == p0 and not many.__dict__.get("_voice_lru")
    # more voices than the LRU holds: all are returned, the LRU keeps the newest
    many.voice_cache_size = 2
    try:
        voices = many.make_voices(specs)
        assert len(voices) == 3 and all(v["prompt_semantic"] is not None for v in voices)
        assert [k[0] for k in many._voice_lru] == [specs[1]["ref_audio_path"], specs[2]["ref_audio_path"]]
    finally:
        del many.voice_cache_size


def test_run_batch_shared_hubert(world):
    from gsv import synthetic as S
    many, single, specs = _fresh(world["many"]), _fresh(world["single"]), world["specs"]
    utt = S.make_utterances(2)
    segs = [{"phones": it["phones"], "bert_features": torch.zeros(1024, len(it["phones"])), "norm_text": it["norm_text"]}
            for it in utt["items"]]
    reqs = [dict(sp, segments=segs, batch_size=2, top_k=1, seed=7 + i, fragment_interval=0.01) for i, sp in enumerate(specs)]
    keep = [dict(r) for r in reqs]
    p0 = _passes(many)
    out = many.run_batch(reqs, shared_hubert=True)
    assert _passes(many) == p0 + 1 and many.cnhuhbert_model.model.last_pass_audios == 3
    assert all(a.keys() == b.keys() and "voice" not in a for a, b in zip(reqs, keep))            # requests are not mutated
    s0 = _passes(single)
    ref = single.run_batch([dict(r) for r in reqs])
    assert _passes(single) == s0
    same_codes = all(torch.equal(many.make_voice(**sp)["prompt_semantic"], single.make_voice(**sp)["prompt_semantic"]) for sp in specs)
    assert len(out) == len(ref) == 3
    for (sr_a, a), (sr_b, b) in zip(out, ref):
        assert sr_a == sr_b == 32000 and a.dtype == b.dtype == np.int16 and a.shape == b.shape and np.abs(a).max() > 0
        if same_codes:
            assert np.array_equal(a, b), "shared_hubert changed more than where the prompt codes come from"
    # it composes with the other shared passes, and a request that brings its voice is left alone
    p1 = _passes(many)
    both = many.run_batch([dict(reqs[0]), dict(reqs[1], voice=many.make_voice(**specs[1]))], shared_hubert=True, shared_sovits=True)
    assert _passes(many) == p1 and len(both) == 2 and both[0][1].shape == out[0][1].shape
