"""`SV` (reference GPT_SoVITS/sv.py:11-32): the speaker-verification embedding of v2Pro / v2ProPlus -- Kaldi fbank (80 bins, 16 kHz)
-> ERes2NetV2(baseWidth=24, scale=4, expansion=4).forward3 -> [B, 20480].  The engine is fp32 whatever `is_half` says (the result
is cast to half like the reference's); weights come from an in-memory state dict or from the reference's checkpoint path loaded
with `weights_only=True` (the file is a plain tensor state dict)."""
from __future__ import annotations

import torch

from .eres2net import kaldi as Kaldi
from .eres2net.ERes2NetV2 import ERes2NetV2

sv_path = "GPT_SoVITS/pretrained_models/sv/pretrained_eres2netv2w24s4ep4.ckpt"


class SV:
    def __init__(self, device, is_half: bool, state_dict=None, path: str = sv_path):
        if state_dict is None:
            state_dict = torch.load(path, map_location="cpu", weights_only=True)
        self.embedding_model = ERes2NetV2(state_dict, device=device, baseWidth=24, scale=4, expansion=4)
        self.device = torch.device(device)
        self.is_half = is_half

    @torch.no_grad()
    def compute_embedding3(self, wav: torch.Tensor) -> torch.Tensor:
        """wav [B, n] at 16 kHz -> [B, 20480]"""
        wav = wav.to(self.device)
        feat = torch.stack([Kaldi.fbank(w.unsqueeze(0), num_mel_bins=80, sample_frequency=16000, dither=0) for w in wav])
        emb = self.embedding_model.forward3(feat)
        return emb.half() if self.is_half else emb

    @torch.no_grad()
    def compute_embedding3_many(self, wavs, max_frames=None):
        """compute_embedding3 for many audios of different lengths: wavs = 1-D or [1, n] tensors at 16 kHz -> one [1, 20480] per
        audio, in order.  The audios of a pass (ERes2NetV2.plan_segments, `max_frames` slot frames, default the model's) stand in one
        sample stream, audio s from sample 160 * slot_start_s, with zeros between them and 240 behind the last: ONE Kaldi fbank
        (four launches) frames the whole stream, and frame slot_start_s + i is frame i of audio s.  The frames past an audio's
        last one are gap rows to forward3_segments.  An audio shorter than the 400-sample window is a ValueError before any
        device work."""
        wavs = [w.reshape(-1) if w.dim() == 2 and w.shape[0] == 1 else w for w in wavs]
        if any(w.dim() != 1 for w in wavs):
            raise ValueError("compute_embedding3_many: 1-D or [1, n] waveforms")
        net = self.embedding_model
        plan = net.plan_segments([1 + (int(w.shape[0]) - 400) // 160 if w.shape[0] >= 400 else 0 for w in wavs], max_frames)
        packed = []
        for ps in plan:
            stream = torch.zeros(160 * ps["frames"] + 240, dtype=torch.float32, device=self.device)
            for s, o in zip(ps["audios"], ps["slot_start"]):
                stream[160 * o:160 * o + wavs[s].shape[0]] = wavs[s].to(self.device, torch.float32)
            packed.append(Kaldi.fbank(stream.unsqueeze(0), num_mel_bins=80, sample_frequency=16000, dither=0))
        emb = net.forward3_segments(packed, plan=plan)
        if self.is_half:
            emb = emb.half()
        return [e.unsqueeze(0) for e in emb]
