"""TEST INFRASTRUCTURE ONLY -- CPU restatement of `CFM.inference(..., inference_cfg_rate=r)` (reference module/models.py:1027-1085)
with classifier-free guidance: oracle/cfm_oracle.py::cfm_inference plus, per Euler step, a second estimate with the prompt
columns zeroed (dit.py:76-78, drop_audio_cond) and the text zeroed BEFORE the positional table and the ConvNeXt stack
(dit.py:44-48, drop_text), combined as v + (v - v_neg) * r (models.py:1081).  The d-embedding is shared between the two
estimates and the null text embedding is cached after the first step, as the reference caches them.  Pinned against the
reference class by tools/gen_golden_cfm_cfg.py (tests/test_cfm_cfg_oracle.py holds it to those goldens)."""
import torch

from oracle.cfm_oracle import dit_forward

CFG_THRESHOLD = 1e-5           # models.py:1063: guidance is active iff rate > 1e-5
RATES = (0.7, 2.0)


def golden_key(rate):
    return "mel_r%02d" % round(rate * 10)


@torch.no_grad()
def cfm_inference_cfg(sd, cfg, mu, prompt, n_timesteps, noise, rate, temperature=1.0):
    """mu [B, T, text_dim]; prompt [B or 1, mel, Tp]; noise [B, mel, T] (the randn draw of models.py:1030) -> [B, mel, T]"""
    B = mu.shape[0]
    x = noise * temperature
    Tp = prompt.shape[-1]
    prompt_x = torch.zeros_like(x)
    prompt_x[..., :Tp] = prompt[..., :Tp]
    x[..., :Tp] = 0
    mu_t = mu.transpose(2, 1)
    t, d = 0.0, 1.0 / n_timesteps
    text_cache = null_text_cache = dt_cache = None
    for _ in range(n_timesteps):
        tt = torch.ones(B) * t
        dd = torch.ones(B) * d
        v, te, dt = dit_forward(sd, cfg, x, prompt_x, tt, dd, mu_t, text_cache, dt_cache)
        text_cache, dt_cache = te, dt
        if rate > CFG_THRESHOLD:
            neg, null_text_cache, _ = dit_forward(sd, cfg, x, torch.zeros_like(prompt_x), tt, dd, torch.zeros_like(mu_t),
                                                  null_text_cache, dt_cache)
            v = v + (v - neg) * rate
        x = x + d * v.transpose(2, 1)
        t = t + d
        x[:, :, :Tp] = 0
    return x
