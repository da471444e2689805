"""GPU: fine-tuned v3 / v4 voices served beside the base model (TTS.add_lora_voice, request key "lora_voice") -- run() and
run_batch(shared_cfm=True) against a second TTS that merged the same LoRA checkpoint into the base model
(init_vits_weights(state=lora, base_state=base), the reference's behaviour), on the small synthetic models in fp32."""
import numpy as np
import pytest
import torch

from gsv import synthetic as S
from test_pipeline_v3_gpu import _build as build_v3
from test_run_batch_cfm_gpu import BAR as SHARED_BAR, BASE, _diff, _voice
from test_run_batch_gpu import _alone, _segs

pytestmark = pytest.mark.gpu
WAVE_BAR = 1e-4         # of full scale (<= 4 int16 LSB): the project's fp32 waveform bar
RANK = 4
OWN = ("ref_enc.", "bridge.", "wns1.")


def _lora_states(vsd, vcfg):
    """voice a: adapters only.  voice b: adapters plus its own ref_enc / bridge / wns1 weights"""
    a = S.make_lora_state_dict(vsd, rank=RANK, seed=3)
    b = S.make_lora_state_dict(vsd, rank=RANK, seed=4)
    own = {k: (v.float() * (1 + 0.2 * S.hash_symmetric("own_" + k, tuple(v.shape), 1.0, 77))).to(v.dtype)
           for k, v in vsd.items() if k.startswith(OWN) and torch.is_floating_point(v)}
    assert len(own) > 10 and {k.split(".")[0] for k in own} == {"ref_enc", "bridge", "wns1"}
    b.update(own)
    return {"a": {"weight": a, "config": vcfg, "lora_rank": RANK}, "b": {"weight": b, "config": vcfg, "lora_rank": RANK}}


def _setup(version):
    tts, _, (vcfg, vsd, _), _ = build_v3(version)
    states = _lora_states(vsd, vcfg)
    merged = {}
    for name, st in states.items():
        m, *_ = build_v3(version)
        m.init_vits_weights(state=st, base_state={"weight": vsd, "config": vcfg})
        merged[name] = m
    return tts, states, merged


@pytest.mark.parametrize("version", ["v3", "v4"])
def test_run_and_run_batch_with_lora_voices(version):
    tts, states, merged = _setup(version)
    va, vb = _voice(0, 8, 6, 14, version), _voice(1, 14, 4, 31, version)
    reqs = [(va, None, dict(BASE, segments=_segs(20, [9, 5]), batch_size=2, seed=3)),
            (va, "a", dict(BASE, segments=_segs(21, [7, 6]), batch_size=2, seed=4)),
            (vb, "b", dict(BASE, segments=_segs(22, [11, 6, 8]), batch_size=2, seed=5)),
            (vb, "a", dict(BASE, segments=_segs(23, [6]), seed=6))]
    # before any voice is added: every request without the key
    before = [_alone(tts, kw, dict(req)) for kw, _, req in reqs]
    enc_before = tts.vits_model
    for name in ("a", "b"):
        tts.add_lora_voice(name, state=states[name])
    assert tts.vits_model is enc_before and tts.vits_model.cfm.estimator.adapter_count() == 2
    assert tts._lora_voices["a"]["engine"] is None, "a file of adapters alone reuses the base encoder engine"
    eb = tts._lora_voices["b"]["engine"]
    assert eb is not None and eb.cfm is tts.vits_model.cfm, "voice b: its own encoder-side engine around the shared DiT"
    # ---- run(): a request without the key is what it was, bit for bit; with it, what the merged model gives
    alone = []
    for r, (kw, name, req) in enumerate(reqs):
        sr0, w0 = _alone(tts, kw, dict(req))
        assert sr0 == before[r][0] and np.array_equal(w0, before[r][1]), f"request {r} without the key changed"
        if name is None:
            alone.append((sr0, w0))
            continue
        sr, w = _alone(tts, kw, dict(req, lora_voice=name))
        srm, wm = _alone(merged[name], kw, dict(req))
        assert sr == srm and w.dtype == wm.dtype == np.int16 and w.shape == wm.shape, f"request {r}: {w.shape} vs {wm.shape}"
        d, moved = _diff(w, wm), _diff(w, w0) if w.shape == w0.shape else 1.0
        print(f"{version} request {r} voice {name}: max |adapted - merged| = {d:.3e} of full scale; |adapted - base| = {moved:.3e}")
        assert d <= WAVE_BAR, f"request {r}: differs from the merged model by {d:.3e} of full scale"
        assert moved >= 100 * WAVE_BAR, f"request {r}: the LoRA voice is the base voice ({moved:.3e})"
        alone.append((sr, w))
    # the chunk-by-chunk path (parallel_infer=False) takes the voice too
    kw, name, req = reqs[2]
    req_np = dict(req, parallel_infer=False)
    _, w = _alone(tts, kw, dict(req_np, lora_voice=name))
    _, wm = _alone(merged[name], kw, dict(req_np))
    assert w.shape == wm.shape and _diff(w, wm) <= WAVE_BAR
    # ---- run_batch(shared_cfm=True): [base, a, b, a] in one flow-matching pass, each against its own run()
    cfm, calls = tts.vits_model.cfm, []
    inner = cfm.inference_rows

    def spy(mu, prompts, *a, **k):
        calls.append(list(k.get("adapters") or []))
        return inner(mu, prompts, *a, **k)
    cfm.inference_rows = spy
    batch = [dict(req, voice=tts.make_voice(**kw), **({} if name is None else {"lora_voice": name})) for kw, name, req in reqs]
    out = tts.run_batch(batch, shared_cfm=True)
    assert len(calls) == 1, f"requests of different LoRA voices and of none share ONE pass, got {len(calls)}"
    slots = {n: tts._lora_voices[n]["slot"] for n in ("a", "b")}
    assert {s for s in calls[0]} == {None, slots["a"], slots["b"]}
    for r, ((sr_a, a), (sr_b, b)) in enumerate(zip(alone, out)):
        assert sr_a == sr_b and a.shape == b.shape, f"request {r}: {a.shape} vs {b.shape}"
        d = _diff(a, b)
        print(f"{version} request {r}: max |shared - run()| = {d:.3e} of full scale over {a.size} samples")
        assert d <= SHARED_BAR and np.abs(a).max() > 0
    # without the key the batch is what it was: no adapters reach the pass
    del calls[:]
    plain = tts.run_batch([dict(req, voice=tts.make_voice(**kw)) for kw, _, req in reqs], shared_cfm=True)
    assert calls == [[]]
    for r, ((_, a), (_, b)) in enumerate(zip(before, plain)):
        assert a.shape == b.shape and _diff(a, b) <= SHARED_BAR
    cfm.inference_rows = inner
    # ---- refused calls
    kw, _, req = reqs[0]
    tts.set_prompt_cache(**kw)
    with pytest.raises(ValueError):
        list(tts.run(dict(req, lora_voice="nobody")))
    with pytest.raises(ValueError):
        tts.run_batch([dict(req, voice=tts.make_voice(**kw), lora_voice="nobody")], shared_cfm=True)
    with pytest.raises(ValueError):
        tts.add_lora_voice("a", state=states["a"])          # the name is taken
    tts.remove_lora_voice("a")
    assert tts.vits_model.cfm.estimator.adapter_count() == 1
    with pytest.raises(ValueError):
        list(tts.run(dict(req, lora_voice="a")))
    with pytest.raises(ValueError):
        tts.remove_lora_voice("a")
    sr, w = _alone(tts, kw, dict(req))
    assert np.array_equal(w, before[0][1]), "the base voice after the refused calls"


def test_v2_model_refuses_lora_voices():
    from test_run_batch_gpu import _build
    tts = _build("v2")
    vcfg = S.small_vits_config()
    vcfg["model"]["inter_channels"] = vcfg["model"]["hidden_channels"]
    dit = S.small_dit_config()
    dit["text_dim"] = 512
    vsd = S.make_vits_v3_state_dict(vcfg, seed=12, dit_cfg=dit)
    with pytest.raises(ValueError):
        tts.add_lora_voice("a", state={"weight": S.make_lora_state_dict(vsd, rank=RANK, seed=3), "config": vcfg, "lora_rank": RANK})
    with pytest.raises(ValueError):
        tts.remove_lora_voice("a")
