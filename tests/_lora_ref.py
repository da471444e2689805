"""Synthetic LoRA adapters for the DiT tests, and the reference of an adapted row: the base weights with the adapter merged in
fp32 by process_ckpt.merge_lora_v3 (the arithmetic tests/test_formats.py pins), for oracle.cfm_oracle / tests/_cfg_ref."""
from __future__ import annotations

import torch

from gsv import process_ckpt as pc
from gsv import synthetic as S

SITES = ("to_q", "to_k", "to_v", "to_out.0")
# Amplitude of the synthetic factors (uniform in [-AMP, AMP] / sqrt(fan-in of the factor)).  Chosen with the oracle on the CPU so
# that a merged row of the small DiT differs from the base row by more than 10 x every bar used (2.2 - 3.7 max-abs, 36 - 63 %
# relative rms against the fp16 bar 0.15 / 3 %) while its output keeps an rms of 1.3 - 1.6, and no larger: the DiT's sensitivity
# to rounding grows steeply with the amplitude.  The plain fp16 engine loaded with the MERGED weights (no adapter code at all)
# is within 0.015 max-abs of the merged oracle at 2.5, within 0.11 at 3.0 and 0.19 - 0.50 away at 3.5 -- beyond the fp16 bar
# on its own -- and the adapted engine measured the same at each amplitude (0.013 / 0.089 / 0.27).
AMP = 2.5


def make_adapter(sd: dict, rank: int, seed: int, amp: float = AMP) -> dict:
    """engine names (`transformer_blocks.<i>.attn.<site>.lora_A|B`) -> fp32 tensors for every adapted Linear of the DiT state
    dict `sd` (keys without the `cfm.estimator.` prefix).  Values are rounded to fp16, as a stored checkpoint holds them, so
    the fp16 engine's copy of the factors is exact."""
    out = {}
    for k, w in sd.items():
        if k.startswith("transformer_blocks.") and any(k.endswith(".attn." + s + ".weight") for s in SITES):
            stem = k[:-len(".weight")]
            a = S.hash_symmetric(stem + "A", (rank, w.shape[1]), amp / w.shape[1] ** 0.5, seed)
            b = S.hash_symmetric(stem + "B", (w.shape[0], rank), amp / rank ** 0.5, seed)
            out[stem + ".lora_A"] = a.half().float()
            out[stem + ".lora_B"] = b.half().float()
    return out


def peft_names(adapter: dict, spelling: str = ".default.weight") -> dict:
    """the adapter as a LoRA checkpoint's `weight` names it (peft, `cfm` wrapped)"""
    return {"cfm.base_model.model.estimator." + k + spelling: v for k, v in adapter.items()}


def merged(sd: dict, adapter: dict, rank: int, alpha=None) -> dict:
    """the DiT state dict with the adapter merged in fp32: what the oracle runs for a row with this adapter"""
    base = {"cfm.estimator." + k: v.float() for k, v in sd.items() if torch.is_tensor(v)}
    out = pc.merge_lora_v3(base, peft_names(adapter), rank, alpha)
    return {k[len("cfm.estimator."):]: v for k, v in out.items()}
