"""Host-side mirror of the reference's `DiT` estimator (GPT_SoVITS/f5_tts/model/backbones/dit.py:88-194).

It holds the hyper-parameters and owns the HIP engine (include/gsv.h `gsv_cfm_*`, csrc/cfm.hip); the Euler loop that
drives it lives in the library too, behind `gsv.module.models.CFM.inference` -- the estimator is never stepped
from Python.  No CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict

import torch

from .... import _lib


class DiT:
    def __init__(self, *, dim, depth=8, heads=8, dim_head=64, dropout=0.1, ff_mult=4, mel_dim=100, text_dim=None,
                 conv_layers=0, long_skip_connection=False, device="cuda", dtype=torch.float16):
        if long_skip_connection:
            raise NotImplementedError("long_skip_connection is never enabled by the reference's v3/v4 models (models.py:1219)")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the gsv DiT runs on an MI355X (cuda/HIP device) only; there is no CPU path")
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        self.dtype = dtype
        self.dim, self.depth, self.heads, self.dim_head, self.ff_mult = dim, depth, heads, dim_head, ff_mult
        self.mel_dim = mel_dim
        self.text_dim = mel_dim if text_dim is None else text_dim
        self.conv_layers = conv_layers
        cfg = _lib.DitConfig(dim, depth, heads, dim_head, ff_mult, mel_dim, self.text_dim, conv_layers)
        with torch.cuda.device(self.device):
            _lib.init(idx)
            h = C.c_void_p()
            _lib.check(_lib.lib().gsv_cfm_create(C.byref(cfg), _lib.dtype_code(dtype), C.byref(h)), "gsv_cfm_create")
            self._h = h
            self.stream = torch.cuda.Stream(device=self.device)
        self._loaded = False
        self._adapters = set()          # live adapter slots (add_adapter)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.lib().gsv_cfm_destroy(h)
            except Exception:
                pass
            self._h = None

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        """keys as in the reference DiT, with or without the `cfm.estimator.` / `estimator.` prefix of a SoVITS checkpoint"""
        l = _lib.lib()

        def items():
            for k, v in state_dict.items():
                for pre in ("cfm.estimator.", "estimator."):
                    if k.startswith(pre):
                        k = k[len(pre):]
                if not torch.is_tensor(v) or k.startswith("rotary_embed") or k.startswith("text_embed.freqs_cis"):
                    continue            # buffers the library rebuilds
                yield k, v

        with torch.cuda.device(self.device):
            _lib.load_tensors(l.gsv_cfm_load_tensor, self._h, items())
            _lib.check(l.gsv_cfm_finalize(self._h), "gsv_cfm_finalize")
        self._loaded = True
        return self

    # ---- LoRA adapters held beside the base weights (gsv_cfm_adapter_*): rows of one pass may each use their own ------------
    ADAPTER_SITES = ("to_q", "to_k", "to_v", "to_out.0")

    def add_adapter(self, adapter: Dict[str, torch.Tensor], rank: int, alpha=None) -> int:
        """`adapter`: `transformer_blocks.<i>.attn.{to_q,to_k,to_v,to_out.0}.lora_{A,B}` -> tensor (lora_A [rank, in], lora_B
        [out, rank]; what process_ckpt.split_lora_v3 returns), all 4 * depth pairs.  `alpha` is peft's lora_alpha, None =
        rank as the reference trains.  Returns the slot CFM.inference_rows(adapters=...) takes; the engine holds at most
        _lib.CFM_MAX_ADAPTERS at once."""
        if not self._loaded:
            raise RuntimeError("DiT.load_state_dict() first")
        rank = int(rank)
        if not 1 <= rank <= _lib.LORA_MAX_RANK:
            raise ValueError(f"LoRA rank must be in [1, {_lib.LORA_MAX_RANK}], got {rank}")
        alpha = float(rank if alpha is None else alpha)
        l = _lib.lib()
        slot = C.c_int(-1)
        with torch.cuda.device(self.device):
            _lib.check(l.gsv_cfm_adapter_begin(self._h, rank, alpha), "gsv_cfm_adapter_begin")
            _lib.load_tensors(l.gsv_cfm_adapter_load_tensor, self._h, adapter.items())
            _lib.check(l.gsv_cfm_adapter_finalize(self._h, C.byref(slot)), "gsv_cfm_adapter_finalize")
        self._adapters.add(slot.value)
        return slot.value

    def remove_adapter(self, slot: int) -> None:
        if slot not in self._adapters:
            raise ValueError(f"no adapter in slot {slot}")
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().gsv_cfm_adapter_remove(self._h, int(slot)), "gsv_cfm_adapter_remove")
        self._adapters.discard(slot)

    def adapter_count(self) -> int:
        return int(_lib.lib().gsv_cfm_adapter_count(self._h))

    def eval(self):
        return self

    def to(self, *a, **k):
        return self
