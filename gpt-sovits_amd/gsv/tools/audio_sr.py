"""`AP_BWE` (reference tools/audio_sr.py:17-53), the 24 kHz -> 48 kHz audio super-resolution that `TTS.run` applies to v3
output when a request sets `super_sampling`, on the HIP engine `gsv_bwe_*` (csrc/bwe.hip): resample, STFT, the two-branch
ConvNeXt model (AP_BWE_main/models/model.py), iSTFT -- no torch compute fallback.

`resample` restates `torchaudio.functional.resample` (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) from its
published definition: torchaudio is not a dependency here, so that step is "parity unpinned" against the package itself.
It is the CPU yardstick of the engine's resampler (tests, tools/gen_golden_bwe.py, tools/bwe_bench.py --cpu-baseline).
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from typing import Optional

import numpy as np
import torch

from .. import _lib

# the reference's default (tools/audio_sr.py:19-22, relative to a reference checkout's root)
DEFAULT_CHECKPOINT = os.path.join("tools", "AP_BWE_main", "24kto48k", "g_24kto48k.zip")
CONFIG_KEYS = ("n_fft", "hop_size", "win_size", "ConvNeXt_channels", "ConvNeXt_layers", "hr_sampling_rate")


def resample(waveform: torch.Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> torch.Tensor:
    """torchaudio.functional.resample(waveform, orig_freq, new_freq) with resampling_method="sinc_interp_hann": the filter is
    built in the waveform's dtype; [..., n] -> [..., ceil(new * n / orig)] (parity unpinned against the package itself)."""
    if orig_freq <= 0 or new_freq <= 0:
        raise ValueError("Original frequency and desired frequecy should be positive")
    if orig_freq == new_freq:
        return waveform
    gcd = math.gcd(int(orig_freq), int(new_freq))
    orig, new = int(orig_freq) // gcd, int(new_freq) // gcd
    dtype, device = waveform.dtype, waveform.device
    base_freq = min(orig, new) * rolloff
    width = math.ceil(lowpass_filter_width * orig / base_freq)
    idx = torch.arange(-width, width + orig, dtype=dtype, device=device)[None, None] / orig
    t = torch.arange(0, -new, -1, dtype=dtype, device=device)[:, None, None] / new + idx
    t *= base_freq
    t = t.clamp_(-lowpass_filter_width, lowpass_filter_width)
    window = torch.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t *= math.pi
    scale = base_freq / orig
    kernels = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t)
    kernels *= window * scale
    shape = waveform.size()
    x = waveform.reshape(-1, shape[-1])
    length = x.shape[-1]
    x = torch.nn.functional.pad(x, (width, width + orig))
    y = torch.nn.functional.conv1d(x[:, None], kernels, stride=orig)
    y = y.transpose(1, 2).reshape(x.shape[0], -1)
    target = int(math.ceil(new * length / orig))
    return y[..., :target].reshape(shape[:-1] + (-1,))


def _cfg_get(h, k):
    return h[k] if isinstance(h, dict) else getattr(h, k)


class AP_BWE:
    """reference tools/audio_sr.py::AP_BWE.  `checkpoint_file` holds {"generator": state_dict} (torch.save), `config.json`
    beside it the model shape; or pass `state={"generator": sd}` and `config` (a dict) directly.  `dtype` is the engine
    dtype: float32 (the reference keeps this model in fp32) or float16 (fp16 GEMM operands, fp32 accumulation; the
    resampler, STFT / iSTFT, norms, log / exp / phase stay fp32)."""

    def __init__(self, device, DictToAttrRecursive=None, checkpoint_file: Optional[str] = None, state: Optional[dict] = None,
                 config=None, dtype=torch.float32):
        if state is None:
            if checkpoint_file is None:
                checkpoint_file = DEFAULT_CHECKPOINT
            if not os.path.exists(checkpoint_file):
                raise FileNotFoundError(f"AP-BWE checkpoint not found: {checkpoint_file} (put g_24kto48k.zip and its "
                                        f"config.json there, see the reference's tools/AP_BWE_main/24kto48k/readme.txt)")
            if config is None:
                config_file = os.path.join(os.path.split(checkpoint_file)[0], "config.json")
                with open(config_file) as f:
                    config = json.load(f)
            state = torch.load(checkpoint_file, map_location="cpu", weights_only=True)
        if config is None:
            raise ValueError("AP_BWE(state=...) needs the model config (the contents of config.json)")
        self.h = DictToAttrRecursive(config) if DictToAttrRecursive is not None and isinstance(config, dict) else config
        self.config = {k: int(_cfg_get(self.h, k)) for k in CONFIG_KEYS}
        self._sd = state["generator"] if "generator" in state else state
        self.dtype = dtype
        self._h = None
        self.device = None
        self.to(device)

    # ---- engine handle ------------------------------------------------------------------------------------------
    def _build(self, device: torch.device):
        from ..module.mel_processing import _dft_basis
        c = self.config
        cfg = _lib.BweConfig()
        cfg.n_fft, cfg.hop_size, cfg.win_size = c["n_fft"], c["hop_size"], c["win_size"]
        cfg.channels, cfg.layers, cfg.hr_sampling_rate = c["ConvNeXt_channels"], c["ConvNeXt_layers"], c["hr_sampling_rate"]
        l = _lib.lib()
        with torch.cuda.device(device):
            _lib.init(device.index)
            h = C.c_void_p()
            _lib.check(l.gsv_bwe_create(C.byref(cfg), _lib.dtype_code(self.dtype), C.byref(h)), "gsv_bwe_create")
            self._h = h
            tensors = dict(self._sd)
            tensors["dft.forward"] = _dft_basis(c["n_fft"], c["win_size"], "cpu")
            tensors["dft.inverse"] = _dft_basis(c["n_fft"], c["win_size"], "cpu", inverse=True)
            _lib.load_tensors(l.gsv_bwe_load_tensor, h, ((k, v) for k, v in tensors.items() if torch.is_tensor(v) and v.numel()))
            _lib.check(l.gsv_bwe_finalize(h), "gsv_bwe_finalize")
            self.stream = torch.cuda.Stream(device=device)

    def _free(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.lib().gsv_bwe_destroy(h)
            except Exception:
                pass
            self._h = None

    def __del__(self):
        self._free()

    def to(self, device=None, dtype=None):
        """reference :35-38 moves the model; here the engine is rebuilt on the new device (or in the new dtype)"""
        device = torch.device(device) if device is not None else self.device
        if device.type != "cuda":
            raise RuntimeError("AP_BWE runs on an MI355X (cuda/HIP device) only; there is no CPU path")
        device = torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())
        dtype = dtype if dtype is not None else self.dtype
        if self._h is None or device != self.device or dtype != self.dtype:
            self._free()
            self.dtype = dtype
            self._build(device)
            self.device = device
        return self

    # ---- inference ----------------------------------------------------------------------------------------------
    def out_len(self, n: int, orig_sampling_rate: int) -> int:
        """samples of the output for n input samples: hop * floor(n_new / hop), n_new = ceil(n * hr / orig)"""
        c = self.config
        n_new = n if orig_sampling_rate == c["hr_sampling_rate"] else -(-n * c["hr_sampling_rate"] // orig_sampling_rate)
        if n_new <= c["n_fft"] // 2:
            raise ValueError(f"{n} samples at {orig_sampling_rate} Hz resample to {n_new}, too short for the reflect padding of "
                             f"{c['n_fft'] // 2} (torch.stft: padding size should be less than the input dimension)")
        return c["hop_size"] * (n_new // c["hop_size"])

    @torch.no_grad()
    def forward_device(self, audio: torch.Tensor, orig_sampling_rate: int) -> torch.Tensor:
        """audio [1, n] or [n] (any device, fp16 / fp32) -> fp32 device tensor [out_len] at hr_sampling_rate"""
        x = audio.reshape(-1)
        n = int(x.shape[0])
        L = self.out_len(n, int(orig_sampling_rate))
        c = self.config
        n_new = n if orig_sampling_rate == c["hr_sampling_rate"] else -(-n * c["hr_sampling_rate"] // int(orig_sampling_rate))
        self._last = (n_new, 1 + n_new // c["hop_size"])
        with torch.cuda.device(self.device):
            if x.dtype not in (torch.float16, torch.float32):
                x = x.float()
            x = x.to(self.device).contiguous()
            out = torch.empty(L, dtype=torch.float32, device=self.device)
            self.stream.wait_stream(torch.cuda.current_stream(self.device))
            rc = _lib.lib().gsv_bwe_forward(self._h, x.data_ptr(), n, _lib.dtype_code(x.dtype), int(orig_sampling_rate), out.data_ptr(),
                                            C.c_void_p(self.stream.cuda_stream))
            if rc == -1:
                raise ValueError(_lib.lib().gsv_last_error().decode(errors="replace"))
            _lib.check(rc, "gsv_bwe_forward")
            torch.cuda.current_stream(self.device).wait_stream(self.stream)
            x.record_stream(self.stream)
            out.record_stream(self.stream)
        return out

    def __call__(self, audio: torch.Tensor, orig_sampling_rate: int):
        """reference :40-53: (waveform float32 numpy at hr_sampling_rate, hr_sampling_rate)"""
        out = self.forward_device(audio, orig_sampling_rate)
        return out.cpu().numpy(), self.config["hr_sampling_rate"]

    def debug_tensor(self, name: str) -> torch.Tensor:
        """stage of the last forward: "resampled" [n_new], "log_amp" / "pha" / "mag_wb" / "pha_wb" [1, bins, T] fp32"""
        l = _lib.lib()
        bins = self.config["n_fft"] // 2 + 1
        with torch.cuda.device(self.device):
            self.stream.synchronize()
            n_new, T = getattr(self, "_last", (0, 0))
            cap = max(n_new if name == "resampled" else bins * T, 1)
            buf = torch.empty(cap, dtype=torch.float32, device=self.device)
            n = C.c_int64()
            _lib.check(l.gsv_bwe_debug_tensor(self._h, name.encode(), buf.data_ptr(), cap, C.byref(n), C.c_void_p(self.stream.cuda_stream)),
                       f"gsv_bwe_debug_tensor({name})")
            self.stream.synchronize()
        t = buf[:n.value].clone()
        return t if name == "resampled" else t.view(1, bins, -1)
