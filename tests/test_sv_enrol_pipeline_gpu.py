"""GPU: TTS.make_voices(shared_sv=True) and run_batch(shared_sv=True) on a v2Pro model: the speaker embeddings of all main and
auxiliary references from one packed ERes2NetV2 pass (SV.compute_embedding3_many) instead of one encoder pass per reference.
The v2Pro TTS of test_set_ref_audio_v2pro_computes_speaker_embedding; three WAV files of 3 s plus 777, 0 and 1234 samples at
32 kHz, the first spec with the third file as an auxiliary reference.  Each embedding is held to the oracle on the voice's own
16 kHz audio at the existing fp16 bar (relative rms 2e-3: the fp16 cast of the result dominates)."""
import copy
import wave

import numpy as np
import pytest
import torch

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
    d = tmp_path_factory.mktemp("sv_enrol")
    files = []
    for i, extra in enumerate((777, 0, 1234)):
        p = str(d / f"ref{i}.wav")
        _write_wav(p, S.make_waveform(3 * 32000 + extra, 3 + i, sr=32000).numpy(), 32000)
        files.append(p)
    pro = copy.deepcopy(S.VITS_V2_CONFIG)
    pro["model"]["version"], pro["model"]["gin_channels"] = "v2Pro", 1024
    t2s = S.make_t2s_state_dict(S.T2S_V2_CONFIG, seed=0, suppress_eos=True)
    hubert = S.make_hubert_state_dict(seed=0)
    sd = S.make_eres2net_state_dict(seed=0)

    def engine(version, cfg):
        tts = TTS({"device": DEV, "is_half": True, "version": version, "max_batch": 4, "max_seq": 600})
        tts.init_t2s_weights(state={"weight": t2s, "config": S.T2S_V2_CONFIG})
        tts.init_vits_weights(state={"weight": S.make_vits_state_dict(cfg, seed=0), "config": cfg})
        tts.init_cnhuhbert_weights(state_dict=hubert)
        tts.configs.max_sec = 0.4
        return tts

    tts = engine("v2Pro", pro)
    tts.init_sv_model(state_dict=sd)
    specs = [dict(ref_audio_path=files[0], prompt_text=TEXT_A, prompt_lang="en", aux_ref_audio_paths=[files[2]]),
             dict(ref_audio_path=files[1], prompt_text=TEXT_B, prompt_lang="en"),
             dict(ref_audio_path=files[2], prompt_text=TEXT_A, prompt_lang="en")]
    return dict(tts=tts, v2=lambda: engine("v2", dict(S.VITS_V2_CONFIG)), specs=specs, files=files, sd=sd, oracle={})


def _fresh(tts):
    tts.__dict__.pop("_voice_lru", None)
    return tts


def _oracle(world, audio16k):
    """the oracle's embedding of one 16 kHz audio, computed once per distinct audio"""
    from oracle import sv_oracle as so
    a = audio16k.float().cpu()
    key = a.numpy().tobytes()
    if key not in world["oracle"]:
        world["oracle"][key] = so.compute_embedding3(world["sd"], a)
    return world["oracle"][key]


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and np.array_equal(a, b)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_make_voices_shared_sv(world):
    tts, specs = _fresh(world["tts"]), world["specs"]
    net = tts.sv_model.embedding_model
    one0, seg0 = net.one_passes, net.seg_passes
    voices = tts.make_voices(specs, shared_sv=True)
    assert net.one_passes == one0 and net.seg_passes == seg0 + 1            # no per-audio pass; three distinct paths, one packed pass
    assert [len(v["sv_emb"]) for v in voices] == [2, 1, 1] and [len(v["refer_spec"]) for v in voices] == [2, 1, 1]
    for vi, v in enumerate(voices):
        for (spec, audio16k), emb in zip(v["refer_spec"], v["sv_emb"]):
            assert audio16k.dtype == torch.float16 and tuple(emb.shape) == (1, 20480) and emb.dtype == torch.float16
            ref = _oracle(world, audio16k)
            rel = float((emb.float().cpu() - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt())
            print(f"[sv enrol] voice {vi}: relative rms {rel:.2e} against the oracle")
            assert rel <= 2e-3
    assert torch.equal(voices[0]["sv_emb"][1], voices[2]["sv_emb"][0])      # the auxiliary reference is the third voice's file
    # every other field is what make_voices without the keyword gives on a fresh LRU
    _fresh(tts)
    one1 = net.one_passes
    plain = tts.make_voices(specs)
    assert net.one_passes == one1 + 4 and net.seg_passes == seg0 + 1         # one encoder pass per main and auxiliary reference
    for v, r in zip(voices, plain):
        assert set(v) == set(r) == set(tts._VOICE_KEYS)
        for k in tts._VOICE_KEYS:
            if k != "sv_emb":
                assert _same(v[k], r[k]), k
        # both are fp16 casts (half an ulp each: 2^-11 of the value) of fp32 results within max-abs 2e-3 of one oracle
        # (test_sv_segments_gpu.py, test_eres2netv2_embedding_matches_reference): 2^-10 of the largest value + 2 x 2e-3
        for a, b in zip(v["sv_emb"], r["sv_emb"]):
            assert float((a.float() - b.float()).abs().max()) <= 2.0 ** -10 * float(b.float().abs().max()) + 4e-3
    assert tts.prompt_cache["ref_audio_path"] is None
    # voices the LRU holds are not encoded again
    seg1 = net.seg_passes
    again = tts.make_voices(specs, shared_sv=True)
    assert net.seg_passes == seg1 and all(x is y for x, y in zip(again, plain))


def test_run_batch_shared_sv(world):
    from gsv import synthetic as S
    tts, specs = _fresh(world["tts"]), world["specs"]
    net = tts.sv_model.embedding_model
    utt = S.make_utterances(2)
    segs = [{"phones": it["phones"], "bert_features": torch.zeros(1024, len(it["phones"])), "norm_text": it["norm_text"]}
            for it in utt["items"]]
    reqs = [dict(sp, segments=segs, batch_size=2, top_k=1, seed=7 + i, fragment_interval=0.01) for i, sp in enumerate(specs)]
    one0, seg0 = net.one_passes, net.seg_passes
    out = tts.run_batch([dict(r) for r in reqs], shared_sovits=True, shared_sv=True)
    assert net.one_passes == one0 and net.seg_passes == seg0 + 1
    _fresh(tts)
    ref = tts.run_batch([dict(r) for r in reqs], shared_sovits=True)
    assert net.seg_passes == seg0 + 1 and net.one_passes == one0 + 4
    assert len(out) == len(ref) == 3
    for (sr_a, a), (sr_b, b) in zip(out, ref):
        assert sr_a == sr_b == 32000 and a.dtype == b.dtype == np.int16 and a.shape == b.shape and np.abs(a).max() > 0


def test_shared_sv_changes_nothing_on_a_v2_model(world):
    v2, specs = world["v2"](), world["specs"]
    assert getattr(v2, "sv_model", None) is None
    a = v2.make_voices(specs, shared_sv=True)
    _fresh(v2)
    b = v2.make_voices(specs)
    for v, r in zip(a, b):
        assert v["sv_emb"] is None and r["sv_emb"] is None
        for k in v2._VOICE_KEYS:
            assert _same(v[k], r[k]), k
