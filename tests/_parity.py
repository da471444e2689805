"""Shared helpers of the bench-shape parity tests (not a conftest: imported explicitly by the tests that use it).

`check_localised` is the localisation check: a global relative RMS averages one broken tile away, so the error is also
measured per window along time and every window is held to the bar.  `dit_v3_chunk_case` is the full-depth DiT case at
the v3 chunk shape, with its CPU oracle output computed once per session and shared by the fp32 and fp16 tests."""
import functools

import numpy as np
import torch


def window_rel_rms(out, ref, window):
    """relative RMS error per run of `window` positions along the last axis (leading axes pooled; the last window may be
    shorter): rms(out - ref) / rms(ref) over each window -> 1-D array"""
    out = np.asarray(out, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert out.shape == ref.shape and out.shape[-1] > 0
    n = out.shape[-1]
    rel = []
    for s in range(0, n, window):
        e = out[..., s:s + window] - ref[..., s:s + window]
        r = ref[..., s:s + window]
        rel.append(np.sqrt((e ** 2).mean()) / max(np.sqrt((r ** 2).mean()), 1e-12))
    return np.array(rel)


def check_localised(out, ref, window, bar, factor, label=""):
    """Assert that no window's relative RMS exceeds 2 x `bar` (the global relative-RMS bar of the comparison) and that the
    worst window is within `factor` of the median window.  Returns (worst, median, worst index, number of windows)."""
    rel = window_rel_rms(out, ref, window)
    worst, med, at = float(rel.max()), float(np.median(rel)), int(rel.argmax())
    print(f"[parity] {label} windows of {window}: worst relative rms {worst * 100:.3f} % (window {at} of {len(rel)}), "
          f"median {med * 100:.3f} %, worst / median {worst / max(med, 1e-30):.2f}")
    assert worst <= 2 * bar, f"{label}: window {at} has relative rms {worst:.3e} > 2 x {bar}"
    assert worst <= factor * med, f"{label}: window {at} has relative rms {worst:.3e} > {factor} x the median {med:.3e}"
    return worst, med, at, len(rel)


def rel_rms(out, ref):
    out, ref = torch.as_tensor(out).double(), torch.as_tensor(ref).double()
    return ((out - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


@functools.lru_cache(maxsize=1)
def dit_v3_chunk_case():
    """BASELINE configs[3] DiT at one chunk: DIT_V3_CONFIG (1024 x 22 blocks, 16 heads x 64), T = 934, Tp = 468, 2 Euler
    steps, hashed inputs and noise -> (cfg, sd, mu, prompt, noise, steps, oracle mel [1, 100, 934]).  The oracle costs
    0.9 TFLOP on the host, so it runs once per session."""
    from gsv import synthetic as S
    from oracle import cfm_oracle
    cfg = dict(S.DIT_V3_CONFIG)
    sd = S.make_dit_state_dict(cfg, seed=9)
    B, T, Tp, steps = 1, 934, 468, 2
    mu = S.hash_symmetric("full_mu", (B, T, cfg["text_dim"]), 1.0, 1)
    prompt = S.hash_symmetric("full_prompt", (1, cfg["mel_dim"], Tp), 1.0, 2)
    noise = S.hash_normal("full_noise", (B, cfg["mel_dim"], T), 3)
    torch.set_num_threads(8)
    ref = cfm_oracle.cfm_inference(sd, cfg, mu, prompt, steps, noise.clone())
    return cfg, sd, mu, prompt, noise, steps, ref
