"""Reference-audio file reading and resampling for `TTS.set_ref_audio` (reference TTS_infer_pack/TTS.py:751-819).

The reference reads with torchaudio.load / librosa.load (soundfile, ffmpeg) and resamples with
torchaudio.transforms.Resample / librosa's soxr: none of them exist in this image.  Here: PCM / float WAV through the
standard library's `wave` module + numpy, and polyphase resampling with scipy.signal.resample_poly (Kaiser-windowed FIR).
PARITY UNPINNED: the resampled waveform differs from the reference's resamplers by their filter designs (a few 1e-3 relative);
everything downstream of the waveform is pinned.
"""
from __future__ import annotations

import math
import wave
from math import gcd
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np


def load_wav(path: str) -> Tuple[np.ndarray, int]:
    """-> (float32 [channels, n] in [-1, 1), sample rate)"""
    with wave.open(path, "rb") as f:
        ch, sw, sr, n = f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()
        raw = f.readframes(n)
    if sw == 1:
        a = (np.frombuffer(raw, dtype=np.uint8).astype(np.float32) - 128.0) / 128.0
    elif sw == 2:
        a = np.frombuffer(raw, dtype="<i2").astype(np.float32) / 32768.0
    elif sw == 3:
        b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v & 0x800000, v - 0x1000000, v)
        a = v.astype(np.float32) / 8388608.0
    elif sw == 4:
        a = np.frombuffer(raw, dtype="<i4").astype(np.float32) / 2147483648.0
    else:
        raise ValueError(f"{path}: unsupported sample width {sw}")
    return a.reshape(-1, ch).T.copy(), sr


def resample(x: np.ndarray, sr_in: int, sr_out: int) -> np.ndarray:
    """x [..., n] float32 -> [..., ceil(n * sr_out / sr_in)]"""
    if sr_in == sr_out:
        return x.astype(np.float32, copy=False)
    from scipy.signal import resample_poly
    g = gcd(int(sr_in), int(sr_out))
    return resample_poly(x.astype(np.float64), sr_out // g, sr_in // g, axis=-1).astype(np.float32)


# ---- the same resampler on the device (gsv_op_resample_poly_seg) -------------------------------------------
# PARITY UNPINNED against torchaudio / soxr, as above: the device path is pinned against `resample` (this module's host resampler).
_filters: Dict[Tuple[int, int], Tuple[np.ndarray, int, int]] = {}
_filters_dev: Dict[Tuple[int, int, str], "torch.Tensor"] = {}


def resample_filter(sr_in: int, sr_out: int) -> Tuple[np.ndarray, int, int]:
    """-> (h float32 [L], up, down): the filter scipy.signal.resample_poly(x, up, down) designs by default, scaled by `up` as it
    applies it; L = 2 * 10 * max(up, down) + 1.  Cached per rate pair."""
    key = (int(sr_in), int(sr_out))
    if key not in _filters:
        from scipy.signal import firwin
        g = gcd(*key)
        up, down = key[1] // g, key[0] // g
        mx = max(up, down)
        h = firwin(2 * 10 * mx + 1, 1.0 / mx, window=("kaiser", 5.0)) * up
        _filters[key] = (h.astype(np.float32), up, down)
    return _filters[key]


def resampled_len(n: int, sr_in: int, sr_out: int) -> int:
    """the length of resample(x [n], sr_in, sr_out): ceil(n * up / down)"""
    g = gcd(int(sr_in), int(sr_out))
    up, down = int(sr_out) // g, int(sr_in) // g
    return (int(n) * up + down - 1) // down


def group_by_rate(rates: Sequence[int]) -> Dict[int, List[int]]:
    """indices of `rates` grouped by value, groups in order of first appearance: one resample launch per group and target rate"""
    groups: Dict[int, List[int]] = {}
    for i, sr in enumerate(rates):
        groups.setdefault(int(sr), []).append(i)
    return groups


def resample_segments(stream, starts: Sequence[int], lens: Sequence[int], sr_in: int, sr_out: int, out=None,
                      out_starts: Optional[Sequence[int]] = None, peak: bool = False):
    """gsv_op_resample_poly_seg over the audios stream[starts[s] : starts[s] + lens[s]] of one fp32 device vector: each resampled
    sr_in -> sr_out as `resample` does (same filter, fp32 accumulation) into out[out_starts[s] : out_starts[s] + m_s], m_s =
    resampled_len(lens[s]).  out=None: a new vector with the outputs back to back (out_starts must be None); else an fp32 device
    vector whose other samples are left as they are.  -> (out, [(start, m_s)], peaks fp32 [n_seg] on the device or None).
    One launch, no synchronisation.  A pair the kernel refuses (its filter or input window is too large) raises RuntimeError."""
    import ctypes as C

    import torch

    from . import _lib
    if int(sr_in) == int(sr_out):
        raise ValueError("resample_segments: sr_in == sr_out is a copy, not a resampling")
    if stream.dtype != torch.float32 or stream.dim() != 1 or stream.device.type != "cuda" or not stream.is_contiguous():
        raise ValueError("resample_segments: the stream is a contiguous 1-D float32 tensor on the GPU")
    h, up, down = resample_filter(sr_in, sr_out)
    dev = stream.device
    key = (int(sr_in), int(sr_out), str(dev))
    if key not in _filters_dev:
        _filters_dev[key] = torch.from_numpy(h).to(dev)
    hd = _filters_dev[key]
    n_seg = len(starts)
    ms = [(int(n) * up + down - 1) // down for n in lens]
    if out is None:
        if out_starts is not None:
            raise ValueError("resample_segments: out_starts without out")
        out_starts = [0] * n_seg
        for s in range(1, n_seg):
            out_starts[s] = out_starts[s - 1] + ms[s - 1]
        out = torch.empty(max(1, sum(ms)), dtype=torch.float32, device=dev)
    elif out_starts is None:
        raise ValueError("resample_segments: out needs out_starts")
    elif out.dtype != torch.float32 or out.dim() != 1 or out.device != dev or not out.is_contiguous():
        raise ValueError("resample_segments: out is a contiguous 1-D float32 tensor on the stream's device")
    pk = torch.empty(max(1, n_seg), dtype=torch.float32, device=dev) if peak else None
    i32 = C.c_int32 * max(1, n_seg)
    with torch.cuda.device(dev):
        _lib.init(dev.index if dev.index is not None else torch.cuda.current_device())
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.lib().gsv_op_resample_poly_seg(
            stream.data_ptr(), int(stream.numel()), hd.data_ptr(), int(hd.numel()), up, down, n_seg, i32(*[int(v) for v in starts]),
            i32(*[int(v) for v in lens]), i32(*[int(v) for v in out_starts]), out.data_ptr(), int(out.numel()),
            pk.data_ptr() if peak else None, st), "gsv_op_resample_poly_seg")
    return out, [(int(a), m) for a, m in zip(out_starts, ms)], pk


RS_TILE, RS_LDS_FLOATS, RS_MAX_FILTER = 1024, 16384, 65535   # csrc/resample.hip: kRsTile, kRsLdsFloats, kRsMaxFilter


def device_resample_supported(sr_in: int, sr_out: int) -> bool:
    """whether gsv_op_resample_poly_seg takes this pair (include/gsv.h: its filter and its input window per tile fit the kernel)"""
    h, up, down = resample_filter(sr_in, sr_out)
    return len(h) <= RS_MAX_FILTER and ((RS_TILE - 1) * down + len(h) - 1) // up + 2 <= RS_LDS_FLOATS


# ---- the output format of a request (gsv_postprocess_groups_rate) ------------------------------------------
ENCODINGS = {"pcm_s16": 0, "mulaw": 1, "alaw": 2}   # include/gsv.h: GSV_OUT_S16, GSV_OUT_MULAW, GSV_OUT_ALAW


def output_rate_supported(sr_in: int, sr_out: int) -> bool:
    """whether gsv_postprocess_groups_rate takes a model at sr_in to sr_out: the same rate (the identity filter), or a pair whose
    filter and input window per tile fit the kernel, the limits of gsv_op_resample_poly_seg"""
    if int(sr_in) <= 0 or int(sr_out) <= 0:
        return False
    return int(sr_in) == int(sr_out) or device_resample_supported(sr_in, sr_out)


def output_filter(sr_in: int, sr_out: int) -> Tuple[np.ndarray, int, int]:
    """-> (h float32 [L], up, down) of gsv_postprocess_groups_rate: resample_filter, or {1.0}, 1, 1 at the same rate"""
    if int(sr_in) == int(sr_out):
        return np.ones(1, dtype=np.float32), 1, 1
    return resample_filter(sr_in, sr_out)


def output_filter_device(sr_in: int, sr_out: int, dev):
    """output_filter with the filter on `dev`, cached per rate pair and device"""
    import torch
    h, up, down = output_filter(sr_in, sr_out)
    key = (int(sr_in), int(sr_out), str(dev))
    if key not in _filters_dev:
        _filters_dev[key] = torch.from_numpy(h).to(dev)
    return _filters_dev[key], up, down


def convert_pcm(pcm: np.ndarray, sr_in: int, sr_out: int, encoding: Optional[str] = None, device="cuda:0",
                loudness: Optional[float] = None, loudness_peak: float = 0.0) -> np.ndarray:
    """int16 audio at sr_in -> the same audio at sr_out as int16 ("pcm_s16", None) or G.711 bytes ("mulaw", "alaw"), through
    one gsv_postprocess_groups_rate call on pcm / 32768 (exact in fp32, peak <= 1: nothing is normalised).  loudness (LUFS,
    -70 .. 0): the audio is one span of gsv_postprocess_groups_loud, metered at sr_in and scaled towards the target under the
    ceiling loudness_peak (dBFS <= 0).  The level is then that of the quantised audio: a caller that
    still has the float sentences uses postprocess_sentences."""
    x = np.ascontiguousarray(pcm, dtype=np.int16).astype(np.float32) / np.float32(32768.0)
    return postprocess_sentences([x], 0, sr_in, sr_out, encoding, device, loudness, "fragment", loudness_peak)[0]


def postprocess_sentences(sentences: Sequence[np.ndarray], gap: int, sr_in: int, sr_out: Optional[int] = None,
                          encoding: Optional[str] = None, device="cuda:0", loudness: Optional[float] = None,
                          loudness_scope: str = "fragment", loudness_peak: float = 0.0) -> Tuple[np.ndarray, list]:
    """The post-processing of one fragment outside a TTS pipeline (inference_cli): float sentences at sr_in, each followed by
    `gap` zeros, through one gsv_postprocess_groups_rate / _loud call -> (int16 or G.711 bytes at sr_out, the loudness reports
    [(lufs, linear gain, limited) per span]).  The peak rule, the saturating int16 and the loudness keywords are those of
    TTS.audio_postprocess: the gain multiplies the float samples, per fragment or per sentence."""
    import ctypes as C

    import torch

    from . import _lib
    sr_out = int(sr_in) if sr_out is None else int(sr_out)
    if encoding is not None and encoding not in ENCODINGS:
        raise ValueError(f"encoding {encoding!r}: one of {', '.join(sorted(ENCODINGS))}")
    if not output_rate_supported(sr_in, sr_out):
        raise ValueError(f"sample_rate {sr_out}: the resampling kernel does not take {sr_in} -> {sr_out}")
    if loudness is not None and loudness_scope not in LOUDNESS_SCOPES:
        raise ValueError(f"loudness_scope {loudness_scope!r}: one of {', '.join(LOUDNESS_SCOPES)}")
    fmt = ENCODINGS[encoding or "pcm_s16"]
    dev = torch.device(device)
    k = len(sentences)
    total = sum(int(x.shape[0]) + int(gap) for x in sentences)
    if total == 0:
        return np.zeros(0, dtype=np.int16 if fmt == 0 else np.uint8), []
    with torch.cuda.device(dev):
        _lib.init(dev.index if dev.index is not None else torch.cuda.current_device())
        xs = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev) for x in sentences]
        hd, up, down = output_filter_device(sr_in, sr_out, dev)
        lens, ptrs = (C.c_int * k)(*[int(x.numel()) for x in xs]), (C.c_void_p * k)(*[x.data_ptr() for x in xs])
        count, gaps = (C.c_int * 1)(k), (C.c_int * 1)(int(gap))
        off = (C.c_longlong * 2)()
        l = _lib.lib()
        spans = []
        if loudness is not None:
            frag = loudness_scope == "fragment"
            spans = [_lib.LoudSpan(f, c, int(frag), float(loudness), float(loudness_peak))
                     for f, c in ([(0, k)] if frag else [(i, 1) for i in range(k)])]
            span_arr = (_lib.LoudSpan * len(spans))(*spans)
            report = torch.empty(16 * len(spans), dtype=torch.uint8, device=dev)
            need = int(l.gsv_postprocess_groups_loud_workspace(lens, k, count, gaps, 1, int(sr_in), len(spans)))
        else:
            need = int(l.gsv_postprocess_groups_rate_workspace(lens, k, 1))
        if need < 0:
            raise ValueError(f"postprocess_sentences: {total} samples at {sr_in} Hz are not taken")
        table = torch.empty(need, dtype=torch.uint8).pin_memory()
        work = torch.empty(need, dtype=torch.uint8, device=dev)
        out = torch.empty(resampled_len(total, sr_in, sr_out), dtype=torch.int16 if fmt == 0 else torch.uint8, device=dev)
        st = torch.cuda.current_stream(dev)
        if spans:
            _lib.check(l.gsv_postprocess_groups_loud(ptrs, lens, k, _lib.GSV_F32, count, gaps, 1, out.data_ptr(), off, table.data_ptr(),
                                                     work.data_ptr(), hd.data_ptr(), int(hd.numel()), up, down, fmt, int(sr_in), span_arr,
                                                     len(spans), report.data_ptr(), C.c_void_p(st.cuda_stream)),
                       "gsv_postprocess_groups_loud")
        else:
            _lib.check(l.gsv_postprocess_groups_rate(ptrs, lens, k, _lib.GSV_F32, count, gaps, 1, out.data_ptr(), off, table.data_ptr(),
                                                     work.data_ptr(), hd.data_ptr(), int(hd.numel()), up, down, fmt,
                                                     C.c_void_p(st.cuda_stream)), "gsv_postprocess_groups_rate")
        host = out.cpu().numpy()                       # waits for the stream: the table is done with
        reports = []
        if spans:
            reports = [(float(r["lufs"]), float(r["gain"]), bool(int(r["flags"]) & _lib.LOUD_LIMITED))
                       for r in report.cpu().numpy().view(_lib.LOUD_REPORT_DTYPE)]
        return host, reports


# ---- loudness normalisation (gsv_postprocess_groups_loud) ---------------------------------------------------
LOUDNESS_SCOPES = ("fragment", "sentence")
_k_weighting: Dict[int, dict] = {}


def k_weighting(rate: int) -> dict:
    """The ITU-R BS.1770 K-weighting for a stream at `rate`, re-derived from the analogue prototype as libebur128 and pyloudnorm
    do, in fp64 and cached per rate: "shelf" and "highpass" = (b [3], a [3]); "A" [4, 4], "B" [4], "C" [4], "D": the cascade as
    one recurrence s' = A s + B x, y = C s + D x (both biquads in transposed direct form II, the arithmetic of the device
    meter); "A16", "A1024", "A4096": the powers of A behind a lane's chunk, a wave and a tile of that meter; "sub_block" =
    round(0.1 rate) samples.  The library derives the same numbers from the rate it is given (csrc/sola.hip, loud_constants)."""
    rate = int(rate)
    if rate <= 0:
        raise ValueError(f"rate {rate}: a sample rate is positive")
    if rate not in _k_weighting:
        f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
        K = math.tan(math.pi * f0 / rate)
        Vh = 10.0 ** (G / 20.0)
        Vb = Vh ** 0.4996667741545416
        a0 = 1.0 + K / Q + K * K
        sb = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
        sa = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
        f0, Q = 38.13547087602444, 0.5003270373238773
        K = math.tan(math.pi * f0 / rate)
        d = 1.0 + K / Q + K * K
        hb = np.array([1.0, -2.0, 1.0])
        ha = np.array([1.0, 2.0 * (K * K - 1.0) / d, (1.0 - K / Q + K * K) / d])
        # y1 = sb0 x + s0; s0' = sb1 x - sa1 y1 + s1; s1' = sb2 x - sa2 y1; y = hb0 y1 + s2; s2' = hb1 y1 - ha1 y + s3; s3' = hb2 y1 - ha2 y
        A = np.array([[-sa[1], 1.0, 0.0, 0.0],
                      [-sa[2], 0.0, 0.0, 0.0],
                      [hb[1] - ha[1] * hb[0], 0.0, -ha[1], 1.0],
                      [hb[2] - ha[2] * hb[0], 0.0, -ha[2], 0.0]])
        B = np.array([sb[1] - sa[1] * sb[0], sb[2] - sa[2] * sb[0], (hb[1] - ha[1] * hb[0]) * sb[0], (hb[2] - ha[2] * hb[0]) * sb[0]])
        Cm = np.array([hb[0], 0.0, 1.0, 0.0])
        _k_weighting[rate] = {"shelf": (sb, sa), "highpass": (hb, ha), "A": A, "B": B, "C": Cm, "D": hb[0] * sb[0],
                              "A16": np.linalg.matrix_power(A, 16), "A1024": np.linalg.matrix_power(A, 1024),
                              "A4096": np.linalg.matrix_power(A, 4096), "sub_block": int(round(0.1 * rate))}
    return _k_weighting[rate]
