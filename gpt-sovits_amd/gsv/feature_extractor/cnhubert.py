"""HuBERT-base content encoder on the HIP library (reference GPT_SoVITS/feature_extractor/cnhubert.py:22-37 wraps
`transformers.HubertModel`; the pipeline calls `cnhubert.model(wav16k.unsqueeze(0))["last_hidden_state"]` on the RAW 16 kHz
waveform, TTS_infer_pack/TTS.py:806-812 -- the Wav2Vec2 feature extractor's normalisation is not applied on that path).

Architecture (HubertConfig defaults = chinese-hubert-base): 7-layer conv feature extractor (kernels 10,3,3,3,3,2,2, strides
5,2,2,2,2,2,2, no bias, GroupNorm(512, 512) after the first conv, GELU), LayerNorm + Linear 512 -> 768, a weight-normed grouped
positional Conv1d(768, 768, k = 128, groups = 16, padding 64, last frame dropped) + GELU added to the sequence, LayerNorm,
12 post-LN encoder layers (12 heads x 64, FFN 3072 GELU).

Host orchestration in Python over the C ABI's single-op entry points, as north_star prescribes: every GEMM / convolution is
`gsv_op_conv1d` (MFMA implicit GEMM, channels-last), attention is `gsv_op_flash_attn64`, normalisations are
`gsv_op_layernorm` / `gsv_op_channel_norm`, the first conv's strided framing is `gsv_op_frame`.  fp16 activations with fp32
accumulation and fp32 normalisation statistics (the reference runs this model in half precision too, TTS.py:329).  There is
no torch compute fallback.  Runs once per reference audio; its output feeds `SynthesizerTrn.extract_latent`.

`HubertModel.batch(wavs)` runs many audios in one packed pass: every audio takes a slot of whole 320-sample
hops in one stream, so that after each strided conv its own frames are a contiguous row range that reads no other audio's
samples; GroupNorm runs per range (`gsv_op_channel_norm_seg`), the positional conv sees the audios 64 zero rows apart
(`gsv_op_gather_rows`), and the 12 layers are the launches above at M = sum T with `gsv_op_flash_attn64_seg`.  The launch count
does not depend on the number of audios, and nothing inside a pass waits for the device.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional

import torch

from .. import _lib

ACT_NONE, ACT_GELU = 0, 7          # csrc/common.h activation codes (GELU = erf form, HubertConfig.hidden_act "gelu")

cnhubert_base_path: Optional[str] = None


class _Out(dict):
    """`model(x)["last_hidden_state"]` and `.last_hidden_state`, like the transformers output object"""
    __getattr__ = dict.__getitem__


class HubertModel:
    conv_kernel = (10, 3, 3, 3, 3, 2, 2)
    conv_stride = (5, 2, 2, 2, 2, 2, 2)

    def __init__(self, device="cuda:0", dtype=torch.float16, hidden=768, layers=12, heads=12, ffn=3072, conv_dim=512,
                 pos_kernel=128, pos_groups=16, eps=1e-5):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("gsv HubertModel runs on an MI355X (cuda/HIP device) only; there is no CPU path")
        if dtype != torch.float16:
            raise NotImplementedError("the HuBERT engine computes in float16 (fused attention is an fp16 kernel)")
        if hidden // heads != 64:
            raise NotImplementedError("head dim must be 64")
        self.dtype, self.hidden, self.layers, self.heads, self.ffn, self.conv_dim = dtype, hidden, layers, heads, ffn, conv_dim
        self.pos_kernel, self.pos_groups, self.eps = pos_kernel, pos_groups, eps
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        _lib.init(idx)
        self.w: Dict[str, torch.Tensor] = {}
        self._loaded = False
        self.passes = 0                  # packed passes issued by batch(), for tests and tools/voice_enrol_bench.py
        self.last_pass_audios = 0        # audios of the newest one

    # ---- weights ---------------------------------------------------------------------------------------------------
    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        """HF `HubertModel.state_dict()` keys (an optional "hubert." prefix is dropped).  Conv weights [Cout, Cin, k] become
        [Cout][k * Cin] (tap-major, cin fastest); q/k/v projections are stacked into one [3 * hidden][hidden] GEMM; the
        positional conv's weight norm (`weight_g` / `weight_v`, or parametrizations original0 / original1, norm over
        dims 0 and 1) is folded."""
        sd = {(k[7:] if k.startswith("hubert.") else k): v.detach().float().cpu() for k, v in sd.items() if torch.is_tensor(v)}
        dev, h = self.device, self.hidden

        def put(name, t, half=True):
            self.w[name] = t.to(dev, torch.float16 if half else torch.float32).contiguous()

        def conv_w(t):          # [Cout, Cin, k] -> [Cout][k * Cin]
            return t.permute(0, 2, 1).reshape(t.shape[0], -1)

        w0 = sd["feature_extractor.conv_layers.0.conv.weight"]                 # [512, 1, 10]
        w0p = torch.zeros(w0.shape[0], 16)
        w0p[:, :10] = w0[:, 0, :]
        put("conv0", w0p)
        put("gn_w", sd["feature_extractor.conv_layers.0.layer_norm.weight"], False)
        put("gn_b", sd["feature_extractor.conv_layers.0.layer_norm.bias"], False)
        for i in range(1, 7):
            put(f"conv{i}", conv_w(sd[f"feature_extractor.conv_layers.{i}.conv.weight"]))
        put("fp_ln_w", sd["feature_projection.layer_norm.weight"], False)
        put("fp_ln_b", sd["feature_projection.layer_norm.bias"], False)
        put("fp_w", sd["feature_projection.projection.weight"])
        put("fp_b", sd["feature_projection.projection.bias"], False)
        pre = "encoder.pos_conv_embed.conv."
        if pre + "weight_g" in sd:
            g, v = sd[pre + "weight_g"], sd[pre + "weight_v"]
        elif pre + "parametrizations.weight.original0" in sd:
            g, v = sd[pre + "parametrizations.weight.original0"], sd[pre + "parametrizations.weight.original1"]
        else:
            g, v = None, sd[pre + "weight"]
        pw = v if g is None else v * (g / v.norm(dim=(0, 1), keepdim=True))      # weight_norm(dim=2)
        put("pos_w", conv_w(pw))                                                   # [768][128 * 48], rows grouped by 48
        put("pos_b", sd[pre + "bias"], False)
        put("enc_ln_w", sd["encoder.layer_norm.weight"], False)
        put("enc_ln_b", sd["encoder.layer_norm.bias"], False)
        for i in range(self.layers):
            p = f"encoder.layers.{i}."
            put(f"l{i}.qkv_w", torch.cat([sd[p + "attention.q_proj.weight"], sd[p + "attention.k_proj.weight"],
                                           sd[p + "attention.v_proj.weight"]], 0))
            put(f"l{i}.qkv_b", torch.cat([sd[p + "attention.q_proj.bias"], sd[p + "attention.k_proj.bias"],
                                           sd[p + "attention.v_proj.bias"]], 0), False)
            put(f"l{i}.o_w", sd[p + "attention.out_proj.weight"])
            put(f"l{i}.o_b", sd[p + "attention.out_proj.bias"], False)
            put(f"l{i}.ln1_w", sd[p + "layer_norm.weight"], False)
            put(f"l{i}.ln1_b", sd[p + "layer_norm.bias"], False)
            put(f"l{i}.f1_w", sd[p + "feed_forward.intermediate_dense.weight"])
            put(f"l{i}.f1_b", sd[p + "feed_forward.intermediate_dense.bias"], False)
            put(f"l{i}.f2_w", sd[p + "feed_forward.output_dense.weight"])
            put(f"l{i}.f2_b", sd[p + "feed_forward.output_dense.bias"], False)
            put(f"l{i}.ln2_w", sd[p + "final_layer_norm.weight"], False)
            put(f"l{i}.ln2_b", sd[p + "final_layer_norm.bias"], False)
        self._loaded = True
        return self

    def eval(self):
        return self

    def half(self):
        return self

    def to(self, device):
        if torch.device(device) != self.device and torch.device(device).type == "cuda" and torch.device(device).index not in (None, self.device.index):
            raise NotImplementedError("create the engine on its device")
        return self

    # ---- ops -------------------------------------------------------------------------------------------------------
    def _conv(self, st, x, T_in, Cin, w, Cout, taps=1, stride=1, pad=0, bias=None, act=ACT_NONE, res=None, T_out=None, ldx=None,
              groups=1):
        l = _lib.lib()
        if T_out is None:
            T_out = (T_in + 2 * pad - taps) // stride + 1
        y = torch.empty(T_out, Cout * groups, dtype=torch.float16, device=self.device)
        d = _lib.ConvDesc()
        d.x, d.w, d.y = x.data_ptr(), w.data_ptr(), y.data_ptr()
        d.bias = bias.data_ptr() if bias is not None else None
        d.res = res.data_ptr() if res is not None else None
        d.T_in, d.T_out, d.Cin, d.Cout, d.taps, d.stride, d.dil, d.pad = T_in, T_out, Cin, Cout, taps, stride, 1, pad
        d.post_act, d.scale = act, 1.0
        if ldx:
            d.ldx = ldx
        if groups > 1:
            d.Z, d.xz, d.wz, d.yz, d.bz = groups, Cin, Cout * taps * Cin, Cout, Cout
            d.ldx, d.ldy = Cin * groups, Cout * groups
        _lib.check(l.gsv_op_conv1d(C.byref(d), _lib.GSV_F16, st), "gsv_op_conv1d")
        return y, T_out

    def _ln(self, st, x, rows, Cn, w, b, res=None):
        y = torch.empty(rows, Cn, dtype=torch.float16, device=self.device)
        _lib.check(_lib.lib().gsv_op_layernorm(x.data_ptr(), res.data_ptr() if res is not None else None, w.data_ptr(), b.data_ptr(),
                                               y.data_ptr(), rows, Cn, self.eps, _lib.GSV_F16, st), "gsv_op_layernorm")
        return y

    def _encoder(self, st, h, T, seg_lens: Optional[List[int]] = None):
        """the 12 post-LN layers on h [T, hidden]; seg_lens: the rows are that many sequences back to back, each attending to its
        own keys (`gsv_op_flash_attn64_seg`), else one sequence (`gsv_op_flash_attn64`)"""
        l, dev, w = _lib.lib(), self.device, self.w
        if seg_lens is None:
            vt = torch.empty(self.hidden * ((T + 31) // 32 * 32), dtype=torch.float16, device=dev)
        else:
            vt = torch.empty(self.hidden * 32 * sum((k + 31) // 32 for k in seg_lens), dtype=torch.float16, device=dev)
            seg = (C.c_int32 * len(seg_lens))(*seg_lens)
        for i in range(self.layers):
            qkv, _ = self._conv(st, h, T, self.hidden, w[f"l{i}.qkv_w"], 3 * self.hidden, bias=w[f"l{i}.qkv_b"])
            att = torch.empty(T, self.hidden, dtype=torch.float16, device=dev)
            if seg_lens is None:
                _lib.check(l.gsv_op_flash_attn64(qkv.data_ptr(), T, self.heads, 0.125, vt.data_ptr(), att.data_ptr(), st),
                           "gsv_op_flash_attn64")
            else:
                _lib.check(l.gsv_op_flash_attn64_seg(qkv.data_ptr(), len(seg_lens), seg, self.heads, 0.125, vt.data_ptr(),
                                                     att.data_ptr(), st), "gsv_op_flash_attn64_seg")
            o, _ = self._conv(st, att, T, self.hidden, w[f"l{i}.o_w"], self.hidden, bias=w[f"l{i}.o_b"], res=h)
            h = self._ln(st, o, T, self.hidden, w[f"l{i}.ln1_w"], w[f"l{i}.ln1_b"])
            f, _ = self._conv(st, h, T, self.hidden, w[f"l{i}.f1_w"], self.ffn, bias=w[f"l{i}.f1_b"], act=ACT_GELU)
            f2, _ = self._conv(st, f, T, self.ffn, w[f"l{i}.f2_w"], self.hidden, bias=w[f"l{i}.f2_b"], res=h)
            h = self._ln(st, f2, T, self.hidden, w[f"l{i}.ln2_w"], w[f"l{i}.ln2_b"])
        return h

    # ---- forward ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def __call__(self, input_values: torch.Tensor, *, stages: Optional[dict] = None, **kw):
        """input_values [1, n] 16 kHz waveform -> {"last_hidden_state": [1, T, hidden]} (T = HF's frame count).  `stages`: a dict
        that receives the [T, hidden] fp16 tensors "pos" (positional conv after GELU) and "enc_in" (the input of layer 0)."""
        if not self._loaded:
            raise RuntimeError("load_state_dict() first")
        if input_values.dim() != 2 or input_values.shape[0] != 1:
            raise ValueError(f"expected a [1, n] waveform, got {tuple(input_values.shape)}")
        n = int(input_values.shape[1])
        if n < 400:
            raise ValueError(f"{n} samples are fewer than the feature extractor's receptive field (400)")
        l, dev, w = _lib.lib(), self.device, self.w
        with torch.cuda.device(dev):
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            x = input_values[0].to(dev, torch.float32).contiguous()
            # conv 0: Conv1d(1, 512, 10, stride 5) as frames [T][16] (10 taps, zero padded) x W [512][16]
            T = (n - 10) // 5 + 1
            fr = torch.empty(T, 16, dtype=torch.float16, device=dev)
            _lib.check(l.gsv_op_frame(x.data_ptr(), n, 10, 5, 0, 16, T, fr.data_ptr(), _lib.GSV_F16, st), "gsv_op_frame")
            h, _ = self._conv(st, fr, T, 16, w["conv0"], self.conv_dim)
            scratch = torch.empty(128 * self.conv_dim, dtype=torch.float32, device=dev)
            hn = torch.empty_like(h)
            _lib.check(l.gsv_op_channel_norm(h.data_ptr(), T, self.conv_dim, w["gn_w"].data_ptr(), w["gn_b"].data_ptr(), 1e-5,
                                             ACT_GELU, scratch.data_ptr(), hn.data_ptr(), _lib.GSV_F16, st), "gsv_op_channel_norm")
            h = hn
            for i in range(1, 7):
                h, T = self._conv(st, h, T, self.conv_dim, w[f"conv{i}"], self.conv_dim, taps=self.conv_kernel[i],
                                  stride=self.conv_stride[i], act=ACT_GELU)
            # feature projection
            h = self._ln(st, h, T, self.conv_dim, w["fp_ln_w"], w["fp_ln_b"])
            h, _ = self._conv(st, h, T, self.conv_dim, w["fp_w"], self.hidden, bias=w["fp_b"])
            # positional conv (grouped, k = 128, pad 64 gives T + 1 frames; HubertSamePadLayer drops the last) + GELU, added
            g = self.pos_groups
            pc, _ = self._conv(st, h, T, self.hidden // g, w["pos_w"], self.hidden // g, taps=self.pos_kernel, pad=self.pos_kernel // 2,
                               bias=w["pos_b"], act=ACT_GELU, T_out=T, groups=g)
            h = self._ln(st, h, T, self.hidden, w["enc_ln_w"], w["enc_ln_b"], res=pc)
            if stages is not None:
                stages["pos"], stages["enc_in"] = pc, h
            h = self._encoder(st, h, T)
        return _Out(last_hidden_state=h.view(1, T, self.hidden))

    # ---- packed pass -----------------------------------------------------------------------------------------------
    HOP = 320                            # product of the conv strides: one output frame per 320 samples
    GAP = 64                             # zero rows between audios in front of the positional conv (its padding)
    MAX_AUDIOS = 8192                    # segments one gsv_op_flash_attn64_seg / gsv_op_channel_norm_seg call takes (include/gsv.h)
    # Slot samples one pass may hold at all.  The conv, GEMM and framing kernels form their element offsets in 64 bits (row * ld as
    # long long in conv_gemm.hip, conv_lds.hip, gemm_lds.hip, gemm_sk.hip and frame_kernel; the stride-2 and grouped convs take
    # conv_gemm_kernel, the only one without a stride-1 or Z = 1 condition), so no kernel sets a limit below the int row counts; this bound keeps the
    # largest array of the pass, conv 0's output of samples / 5 rows x 512 channels, below 2^31 elements all the same, so that the
    # pass stays correct even where a kernel or a caller indexes it with an int.  21.8 minutes of audio.
    PASS_LIMIT = 5 * (2 ** 31 // 512)
    # Slot samples of one packed pass unless the caller says otherwise, from the sweep of tools/voice_enrol_bench.py on an MI355X
    # (32 audios of 10 s = 5.19 M slot samples; ms per batch() call, median of 7, and peak workspace): 2^19 -> 36.3 (11 passes,
    # 0.22 GB), 2^20 -> 28.5 (6, 0.41 GB), 2^21 -> 24.1 (3, 0.83 GB), 2^22 -> 23.5 (2, 1.6 GB), 2^23 -> 21.9 (1, 2.1 GB).  Beyond 2^21
    # a doubling buys under 3 % and costs twice the workspace.
    MAX_SAMPLES = 2 ** 21

    @classmethod
    def pack_plan(cls, lengths) -> dict:
        """The layout of one packed pass over audios of `lengths` samples: host arithmetic only.  Audio s takes a slot of
        K_s = ceil(n_s / 320) * 320 samples that starts at sample 320 * k_s, k_s = sum_{s' < s} K_s' / 320.  After conv i its own frames
        are the rows from k_s * 320 / (stride product so far): 64 k_s after conv 0 (T0_s rows), k_s after conv 6 (T_s rows).  Keys:
          n_audio, lengths, k, slot_off [samples], samples (sum K_s), T0, T, rows0 (conv 0's output rows), rows (conv 6's)
          cn_start, cn_len    the GroupNorm segments: rows 64 k_s .. + T0_s of conv 0's output
          gather_pad          int32 [sum T + 64 (n - 1)]: the packed row of each row of the positional conv's input, -1 in the
                              64 rows between two audios
          gather_dense        int32 [sum T]: the rows of that layout which belong to an audio, in order
          row0                first row of each audio in the dense [sum T, hidden] matrix"""
        lengths = [int(n) for n in lengths]
        if not lengths:
            raise ValueError("pack_plan: no audio")
        if len(lengths) > cls.MAX_AUDIOS:
            raise ValueError(f"pack_plan: {len(lengths)} audios exceed the {cls.MAX_AUDIOS} segments of one pass")
        for n in lengths:
            if n < 400:
                raise ValueError(f"{n} samples are fewer than the feature extractor's receptive field (400)")
        hop, gap = cls.HOP, cls.GAP
        k, acc = [], 0
        for n in lengths:
            k.append(acc)
            acc += (n + hop - 1) // hop
        samples = acc * hop
        if samples >= cls.PASS_LIMIT:
            raise ValueError(f"pack_plan: {samples} slot samples reach the limit of one pass ({cls.PASS_LIMIT})")
        T0 = [(n - 10) // 5 + 1 for n in lengths]
        T = [(n - 400) // hop + 1 for n in lengths]
        pad_rows, dense, row0, at, m = [], [], [], 0, 0
        for s, (ks, ts) in enumerate(zip(k, T)):
            if s:
                pad_rows += [-1] * gap
                at += gap
            pad_rows += range(ks, ks + ts)
            dense += range(at, at + ts)
            row0.append(m)
            at += ts
            m += ts
        return {"n_audio": len(lengths), "lengths": lengths, "k": k, "slot_off": [hop * ks for ks in k], "samples": samples,
                "T0": T0, "T": T, "rows0": samples // 5 - 1, "rows": acc - 1,
                "cn_start": [64 * ks for ks in k], "cn_len": T0,
                "gather_pad": torch.tensor(pad_rows, dtype=torch.int32), "gather_dense": torch.tensor(dense, dtype=torch.int32),
                "row0": row0}

    @classmethod
    def pack_passes(cls, lengths, max_samples: Optional[int] = None) -> List[List[int]]:
        """input-order groups of audio indices, one per pass: at most `max_samples` slot samples and MAX_AUDIOS audios each.  An audio
        is never split; one whose slot alone exceeds max_samples gets a pass of its own if it is below PASS_LIMIT."""
        max_samples = cls.MAX_SAMPLES if max_samples is None else int(max_samples)
        if max_samples < 400 or max_samples >= cls.PASS_LIMIT:
            raise ValueError(f"max_samples = {max_samples}: a pass holds 400 .. {cls.PASS_LIMIT - 1} slot samples")
        groups, group, held = [], [], 0
        for i, n in enumerate(lengths):
            n = int(n)
            if n < 400:
                raise ValueError(f"{n} samples are fewer than the feature extractor's receptive field (400)")
            slot = (n + cls.HOP - 1) // cls.HOP * cls.HOP
            if slot >= cls.PASS_LIMIT:
                raise ValueError(f"an audio of {n} samples exceeds the limit of one pass ({cls.PASS_LIMIT} slot samples)")
            if group and (held + slot > max_samples or len(group) == cls.MAX_AUDIOS):
                groups.append(group)
                group, held = [], 0
            group.append(i)
            held += slot
        if group:
            groups.append(group)
        return groups

    @torch.no_grad()
    def _packed_pass(self, wavs: List[torch.Tensor], stages: Optional[dict]) -> List[torch.Tensor]:
        """one pass over 1-D waveforms: [1, T_s, hidden] views of one dense device matrix, in order"""
        plan = self.pack_plan([int(x.numel()) for x in wavs])
        l, dev, w, n = _lib.lib(), self.device, self.w, plan["n_audio"]
        N, R0, R, Ts = plan["samples"], plan["rows0"], plan["rows"], plan["T"]
        M, Mp = sum(Ts), int(plan["gather_pad"].numel())
        idx_host = torch.cat([plan["gather_pad"], plan["gather_dense"]]).pin_memory()
        with torch.cuda.device(dev):
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            if all(x.device.type == "cpu" for x in wavs):           # one staging buffer, one upload
                host = torch.zeros(N, dtype=torch.float32, pin_memory=True)
                for x, off in zip(wavs, plan["slot_off"]):
                    host[off:off + x.numel()] = x
                x = host.to(dev, non_blocking=True)
            else:
                x = torch.zeros(N, dtype=torch.float32, device=dev)
                for xs, off in zip(wavs, plan["slot_off"]):
                    x[off:off + xs.numel()].copy_(xs, non_blocking=True)
            idx = idx_host.to(dev, non_blocking=True)
            fr = torch.empty(R0, 16, dtype=torch.float16, device=dev)
            _lib.check(l.gsv_op_frame(x.data_ptr(), N, 10, 5, 0, 16, R0, fr.data_ptr(), _lib.GSV_F16, st), "gsv_op_frame")
            h, _ = self._conv(st, fr, R0, 16, w["conv0"], self.conv_dim)
            del fr
            chunks = sum((t + 255) // 256 for t in plan["cn_len"])
            scratch = torch.empty(2 * self.conv_dim * (chunks + n), dtype=torch.float32, device=dev)
            hn = torch.empty_like(h)
            _lib.check(l.gsv_op_channel_norm_seg(h.data_ptr(), R0, self.conv_dim, n, (C.c_int32 * n)(*plan["cn_start"]),
                                                 (C.c_int32 * n)(*plan["cn_len"]), w["gn_w"].data_ptr(), w["gn_b"].data_ptr(), 1e-5,
                                                 ACT_GELU, scratch.data_ptr(), hn.data_ptr(), _lib.GSV_F16, st),
                       "gsv_op_channel_norm_seg")
            h, T = hn, R0
            del hn
            for i in range(1, 7):
                h, T = self._conv(st, h, T, self.conv_dim, w[f"conv{i}"], self.conv_dim, taps=self.conv_kernel[i],
                                  stride=self.conv_stride[i], act=ACT_GELU)
            assert T == R, (T, R)
            h = self._ln(st, h, R, self.conv_dim, w["fp_ln_w"], w["fp_ln_b"])
            h, _ = self._conv(st, h, R, self.conv_dim, w["fp_w"], self.hidden, bias=w["fp_b"])
            # the audios 64 zero rows apart: the positional conv's own padding covers both ends
            hp = torch.empty(Mp, self.hidden, dtype=torch.float16, device=dev)
            _lib.check(l.gsv_op_gather_rows(h.data_ptr(), R, idx[:Mp].data_ptr(), Mp, self.hidden, hp.data_ptr(), _lib.GSV_F16, st),
                       "gsv_op_gather_rows")
            g = self.pos_groups
            pc, _ = self._conv(st, hp, Mp, self.hidden // g, w["pos_w"], self.hidden // g, taps=self.pos_kernel,
                               pad=self.pos_kernel // 2, bias=w["pos_b"], act=ACT_GELU, T_out=Mp, groups=g)
            hp = self._ln(st, hp, Mp, self.hidden, w["enc_ln_w"], w["enc_ln_b"], res=pc)
            h = torch.empty(M, self.hidden, dtype=torch.float16, device=dev)
            _lib.check(l.gsv_op_gather_rows(hp.data_ptr(), Mp, idx[Mp:].data_ptr(), M, self.hidden, h.data_ptr(), _lib.GSV_F16, st),
                       "gsv_op_gather_rows")
            if stages is not None:
                pos = torch.empty(M, self.hidden, dtype=torch.float16, device=dev)
                _lib.check(l.gsv_op_gather_rows(pc.data_ptr(), Mp, idx[Mp:].data_ptr(), M, self.hidden, pos.data_ptr(), _lib.GSV_F16,
                                                st), "gsv_op_gather_rows")
                stages.setdefault("_pos", []).append(pos)
                stages.setdefault("_enc_in", []).append(h)
            h = self._encoder(st, h, M, Ts)
        self.passes += 1
        self.last_pass_audios = n
        return [rows.view(1, t, self.hidden) for rows, t in zip(h.split(Ts), Ts)]

    def batch(self, wavs, max_samples: Optional[int] = None, stages: Optional[dict] = None) -> List[torch.Tensor]:
        """last hidden state of every audio, one [1, T_s, hidden] fp16 device tensor each, in input order.  `wavs`: 1-D or [1, n]
        16 kHz waveforms on the host or the device.  Audios are packed in input order into passes of at most `max_samples` slot
        samples (MAX_SAMPLES) and MAX_AUDIOS audios; an audio is never split.  `stages`: a dict that receives "pos" and "enc_in"
        as in __call__, [sum T_s, hidden] in input order."""
        if not self._loaded:
            raise RuntimeError("load_state_dict() first")
        flat = []
        for x in wavs:
            if x.dim() == 2 and x.shape[0] == 1:
                x = x[0]
            if x.dim() != 1:
                raise ValueError(f"expected a 1-D or [1, n] waveform, got {tuple(x.shape)}")
            flat.append(x)
        groups = self.pack_passes([int(x.numel()) for x in flat], max_samples)     # every length is checked before any launch
        out: List[torch.Tensor] = []
        for grp in groups:
            out += self._packed_pass([flat[i] for i in grp], stages)
        if stages is not None:
            for key in ("pos", "enc_in"):
                parts = stages.pop("_" + key, [])
                if parts:
                    stages[key] = parts[0] if len(parts) == 1 else torch.cat(parts)
        return out


class CNHubert:
    """reference feature_extractor/cnhubert.py:22-37: `.model` is the HubertModel; weights come from `base_path`
    (`pytorch_model.bin` read with a non-executing loader, or `model.safetensors`)."""

    def __init__(self, base_path: Optional[str] = None, device="cuda:0", dtype=torch.float16, state_dict: Optional[dict] = None):
        self.model = HubertModel(device=device, dtype=dtype)
        if state_dict is None:
            base_path = base_path or cnhubert_base_path
            if base_path is None or not os.path.exists(base_path):
                raise FileNotFoundError(base_path)
            st = os.path.join(base_path, "model.safetensors")
            if os.path.exists(st):
                from safetensors.torch import load_file
                state_dict = load_file(st)
            else:
                state_dict = torch.load(os.path.join(base_path, "pytorch_model.bin"), map_location="cpu", weights_only=True)
        self.model.load_state_dict(state_dict)

    def eval(self):
        return self

    def half(self):
        return self

    def to(self, device):
        return self

    def forward(self, x):
        return self.model(x)["last_hidden_state"]

    def batch(self, wavs, max_samples: Optional[int] = None, stages: Optional[dict] = None):
        return self.model.batch(wavs, max_samples=max_samples, stages=stages)

    __call__ = forward


def get_model():
    return CNHubert()
