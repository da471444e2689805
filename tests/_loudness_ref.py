"""The fp64 mirror of the loudness meter and gain of gsv_postprocess_groups_loud / gsv_op_loudness (include/gsv.h, DESIGN.md
section 4v): ITU-R BS.1770 K-weighting re-derived for the stream's rate, a sequential scipy.signal.lfilter over the materialised
span, 100 ms sub-block energies, 400 ms gating blocks with 75 % overlap, the absolute and the relative gate, the gain and its
ceiling.  The coefficient formulas are restated here and not imported from the product."""
import math

import numpy as np
from scipy.signal import lfilter

LIMITED, NAN, SILENT = 1, 2, 4          # the report's flags

# the seven numbers ITU-R BS.1770-4 prints for 48 kHz (tables 1 and 2; b of the high-pass is 1, -2, 1)
BS1770_48K = {"shelf_b": (1.53512485958697, -2.69169618940638, 1.19839281085285), "shelf_a": (-1.69065929318241, 0.73248077421585),
              "hp_a": (-1.99004745483398, 0.99007225036621)}


def k_coefficients(rate):
    """-> (b_shelf [3], a_shelf [3], b_hp [3], a_hp [3]) in fp64"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / rate)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    b1 = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    a1 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / rate)
    d = 1.0 + K / Q + K * K
    b2 = np.array([1.0, -2.0, 1.0])
    a2 = np.array([1.0, 2.0 * (K * K - 1.0) / d, (1.0 - K / Q + K * K) / d])
    return b1, a1, b2, a2


def norm_sentence(x):
    """the "in T" normalisation of the post-processing kernels: x / peak in x's dtype when the peak exceeds 1 and x holds no NaN;
    -> (fp32 samples, peak as float, has_nan)"""
    x = np.asarray(x)
    if x.size == 0:
        return np.zeros(0, dtype=np.float32), 0.0, False
    a = np.abs(x.astype(np.float32))
    if np.isnan(a).any():
        return x.astype(np.float32), float("nan"), True
    peak = a.max()
    if peak > 1.0:
        x = (x.astype(np.float32) / np.float32(peak)).astype(x.dtype)
    return x.astype(np.float32), float(peak), False


def span_stream(sentences, gap, gaps=True):
    """the samples of a span: concat_i [norm(x_i), gap zeros when `gaps`] in fp32"""
    parts = []
    for x in sentences:
        parts.append(norm_sentence(x)[0])
        if gaps and gap:
            parts.append(np.zeros(gap, dtype=np.float32))
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32)


def level(z):
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def meter(stream, rate):
    """-> dict: energies [ceil(N / s)] (the last one the trailing partial sub-block), blocks z [nb], their levels, the masks of
    both gates, the relative gate, lufs"""
    x = np.asarray(stream, dtype=np.float64)
    N = x.shape[0]
    s = int(round(0.1 * rate))
    b1, a1, b2, a2 = k_coefficients(rate)
    y = lfilter(b2, a2, lfilter(b1, a1, x)) if N else x
    sq = y * y
    Jt, J = -(-N // s), N // s
    energies = np.array([sq[j * s:(j + 1) * s].sum() for j in range(Jt)])
    if J >= 4:
        z = np.array([energies[b:b + 4].sum() / (4.0 * s) for b in range(J - 3)])
    elif N > 0:
        z = np.array([sq.sum() / N])
    else:
        z = np.zeros(0)
    lv = level(z)
    keep_abs = lv > -70.0
    out = {"energies": energies, "z": z, "levels": lv, "abs": keep_abs, "rel": np.zeros_like(keep_abs), "gate": None,
           "lufs": -math.inf, "s": s, "J": J}
    if keep_abs.any():
        gate = float(level(z[keep_abs].mean())) - 10.0
        keep = keep_abs & (lv > gate)
        out["gate"], out["rel"] = gate, keep
        if keep.any():
            out["lufs"] = float(level(z[keep].mean()))
    return out


def gate_margin(m):
    """the smallest distance in LU of any block of meter() m to either gate (inf when there is no block or no gate)"""
    lv = m["levels"]
    lv = lv[np.isfinite(lv)]
    if lv.size == 0:
        return math.inf
    d = np.abs(lv + 70.0).min()
    if m["gate"] is not None:
        d = min(d, np.abs(lv - m["gate"]).min())
    return float(d)


def span_gain(lufs, target, peak_db, sentences):
    """-> (gain as fp64, flags).  target None or NaN: meter only"""
    flags, P = 0, 0.0
    for x in sentences:
        _, peak, nan = norm_sentence(x)
        if nan:
            flags |= NAN
        else:
            P = max(P, min(peak, 1.0))
    if not flags and lufs == -math.inf:
        flags |= SILENT
    g = 1.0
    if not flags and target is not None and not math.isnan(target):
        g = 10.0 ** ((float(target) - lufs) / 20.0)
        c = 10.0 ** (float(peak_db) / 20.0)
        if g * P > c:
            g, flags = c / P, flags | LIMITED
    return g, flags


def s16(y):
    """GSV_OUT_S16 on the host: y * 32768 in fp32, clamped to [-32768, 32767], truncated toward zero"""
    q = np.clip(np.asarray(y, dtype=np.float32) * np.float32(32768.0), np.float32(-32768.0), np.float32(32767.0))
    return np.trunc(q).astype(np.int16)
