"""CPU: a v3 / v4 LoRA checkpoint taken apart for a voice served beside the base model (process_ckpt.split_lora_v3) against
the merge that tests/test_formats.py pins (merge_lora_v3), and the request key "lora_voice" in the option resolver and the
flow-matching planner.  No compute is called here."""
import inspect
from types import SimpleNamespace

import pytest
import torch

from gsv import process_ckpt as pc
from gsv import synthetic as S
from gsv.TTS_infer_pack.TTS import TTS

RANK = 4
SITES = ("to_q", "to_k", "to_v", "to_out.0")


@pytest.fixture(scope="module")
def ckpt():
    vcfg = S.small_vits_config()
    vcfg["model"]["inter_channels"] = vcfg["model"]["hidden_channels"]
    dit = S.small_dit_config()
    dit["text_dim"] = 512
    base = S.make_vits_v3_state_dict(vcfg, seed=12, dit_cfg=dit)
    return base, S.make_lora_state_dict(base, rank=RANK, seed=3), dit


def _rebuild(base, adapter, scale):
    out = dict(base)
    for k in adapter:
        if k.endswith(".lora_A"):
            stem = k[:-len(".lora_A")]
            w = base["cfm.estimator." + stem + ".weight"]
            out["cfm.estimator." + stem + ".weight"] = (w.float() + scale * (adapter[stem + ".lora_B"] @ adapter[k])).to(w.dtype)
    return out


@pytest.mark.parametrize("alpha", [None, 8])
def test_split_parts_rebuild_the_merged_weights(ckpt, alpha):
    base, lw, dit = ckpt
    adapter, overrides = pc.split_lora_v3(lw, RANK, alpha)
    assert overrides == {}
    want_names = {f"transformer_blocks.{i}.attn.{s}.lora_{ab}" for i in range(dit["depth"]) for s in SITES for ab in "AB"}
    assert set(adapter) == want_names
    assert all(t.dtype == torch.float32 for t in adapter.values())
    merged = pc.merge_lora_v3(base, lw, RANK, alpha)
    rebuilt = _rebuild(base, adapter, (RANK if alpha is None else alpha) / RANK)
    assert set(rebuilt) == set(merged)
    for k in merged:
        assert torch.equal(rebuilt[k], merged[k]), k


def test_overrides_are_returned_untouched_under_the_base_names(ckpt):
    base, lw, _ = ckpt
    extra = {k: base[k] + 1 for k in base if k.startswith(("ref_enc.", "bridge.", "wns1."))}
    assert extra
    frozen = "cfm.base_model.model.estimator.transformer_blocks.0.attn.to_q.base_layer.weight"
    plain = "cfm.base_model.model.estimator.proj_out.bias"
    lw2 = dict(lw, **extra)
    lw2[frozen] = base["cfm.estimator.transformer_blocks.0.attn.to_q.weight"]
    lw2[plain] = base["cfm.estimator.proj_out.bias"]
    adapter, overrides = pc.split_lora_v3(lw2, RANK)
    assert set(adapter) == set(pc.split_lora_v3(lw, RANK)[0])
    assert set(overrides) == set(extra) | {"cfm.estimator.transformer_blocks.0.attn.to_q.weight", "cfm.estimator.proj_out.bias"}
    for k, v in extra.items():
        assert overrides[k] is v
    assert overrides["cfm.estimator.proj_out.bias"] is lw2[plain]
    # the same entries are what the merge lays over the base weights
    merged = pc.merge_lora_v3(base, lw2, RANK)
    for k, v in overrides.items():
        assert merged[k] is v


def test_both_peft_spellings(ckpt):
    _, lw, _ = ckpt
    short = {k.replace(".default.weight", ".weight"): v for k, v in lw.items()}
    assert set(short) != set(lw)
    a0, _ = pc.split_lora_v3(lw, RANK)
    a1, _ = pc.split_lora_v3(short, RANK)
    assert set(a0) == set(a1) and all(torch.equal(a0[k], a1[k]) for k in a0)
    # without the peft prefix, as a state dict of the unwrapped module names them
    bare = {("cfm." + k[len("cfm.base_model.model."):]).replace(".default.weight", ".weight"): v for k, v in lw.items()}
    a2, _ = pc.split_lora_v3(bare, RANK)
    assert set(a2) == set(a0) and all(torch.equal(a0[k], a2[k]) for k in a0)


def test_errors_are_the_merges(ckpt):
    base, lw, _ = ckpt
    ka = "cfm.base_model.model.estimator.transformer_blocks.0.attn.to_q.lora_A.default.weight"
    kb = ka.replace("lora_A", "lora_B")
    cases = []
    cases.append((KeyError, {k: v for k, v in lw.items() if k != kb}, RANK))                     # a lora_A without its lora_B
    cases.append((ValueError, lw, 8))                                                            # rank differs from lora_rank
    cases.append((ValueError, {"enc_p.ssl_proj.weight": base["enc_p.ssl_proj.weight"]}, RANK))   # no pairs at all
    bad = dict(lw)
    bad["cfm.base_model.model.estimator.nowhere.to_q.lora_A.default.weight"] = lw[ka]
    bad["cfm.base_model.model.estimator.nowhere.to_q.lora_B.default.weight"] = lw[kb]
    cases.append((KeyError, bad, RANK))                                                          # not a base parameter
    for exc, weights, rank in cases:
        with pytest.raises(exc):
            pc.merge_lora_v3(base, weights, rank)
        with pytest.raises(exc):
            pc.split_lora_v3(weights, rank)
    with pytest.raises(ValueError):
        pc.split_lora_v3(lw, RANK, lora_alpha=0)


def test_request_options_carry_the_key():
    assert TTS._request_options({"lora_voice": "a"})["lora_voice"] == "a"
    # absent or None is the base model: the options are the ones they were
    plain = TTS._request_options({})
    assert plain.get("lora_voice") is None and TTS._request_options({"lora_voice": None}) == plain
    assert dict(TTS._request_options({"lora_voice": "a", "top_k": 3}), lora_voice=None) == dict(TTS._request_options({"top_k": 3}), lora_voice=None)
    # resolved once: an unknown name is refused by _resolve_options, before any stage runs
    stub = SimpleNamespace(configs=SimpleNamespace(version="v3", use_vocoder=True), _request_options=TTS._request_options,
                           _lora_voices={"a": dict(slot=3, engine=None)}, vits_model="base")
    stub._lora_voice = lambda name: TTS._lora_voice(stub, name)
    assert TTS._resolve_options(stub, {"lora_voice": "a"})["lora_voice"] == "a"
    assert TTS._lora_voice(stub, "a") == ("base", 3) and TTS._lora_voice(stub, None) == ("base", None)
    with pytest.raises(ValueError):
        TTS._resolve_options(stub, {"lora_voice": "nobody"})
    for fn in (TTS.using_vocoder_synthesis, TTS.using_vocoder_synthesis_batched_infer):
        assert inspect.signature(fn).parameters["lora_voice"].default is None


def test_plan_cfm_does_not_split_by_voice():
    vc = {"T_ref": 20, "T_chunk": 48, "overlapped_len": 4, "upsample_rate": 256, "sr": 24000}
    stub = SimpleNamespace(configs=SimpleNamespace(use_vocoder=True), vocoder_configs=vc, cfm_max_rows=5, _chunk_cuts=TTS._chunk_cuts)
    shapes = [(14, [150], {}), (20, [90, 30], {}), (17, [100], {"inference_cfg_rate": 0.7}), (14, [60], {"sample_steps": 8}),
              (20, [40], {})]
    voices = ["a", None, "b", "a", "c"]

    def plans(with_key):
        return [dict(T_min=t, cfm_folds=list(f), opts=TTS._request_options(dict(o, **({"lora_voice": v} if with_key and v else {}))))
                for (t, f, o), v in zip(shapes, voices)]
    assert TTS.plan_cfm(stub, plans(True)) == TTS.plan_cfm(stub, plans(False))
    assert any(len({voices[r] for r, _, _ in rows}) > 1 for rows in TTS.plan_cfm(stub, plans(True))), "voices share a pass"
