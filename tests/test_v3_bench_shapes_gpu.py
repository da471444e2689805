"""GPU: the v3 / v4 path (BASELINE configs[3]) in its production dtype at the shapes the benchmark times, against the CPU
oracles (oracle/cfm_oracle.py, oracle/vocoder_oracle.py; both pinned against the reference classes).

These shapes select kernels that the reduced cases never launch: at T = 934 the QKV projection of the DiT (192 tiles of
128 x 128) takes the 8-wave LDS tile GEMM and the other Linear layers the t64 GEMM, with the weights of blocks >= 8 loaded
non-temporally (`gemm_t64_f16_kernel<true, 128>`); fp16 attention applies the rotary embedding inside the flash / V^T
launch; B = 8 chunks (7472 rows) put every Linear on the tile GEMM and address each chunk by its row offset; 32 Euler
steps walk the whole modulation table; and the vocoders at length run many anti-alias tiles (BigVGAN) and `conv_wide`
(128 channels, T >= 16 384), the persistent 64-channel narrow conv (T >= 16 384), the fused 32 / 16-channel ResBlock pairs
and the persistent `conv_narrow<16>` conv_post (T >= 4096) of the v4 HiFi-GAN.

Bars: fp32 as the reduced cases (DiT max-abs <= 2e-3, vocoders <= 2e-4); fp16 DiT relative RMS <= 3 % and max-abs <= 0.15,
fp16 vocoders relative RMS <= 5 % and max-abs <= 3e-2.  Every fp16 comparison also passes the
localisation check of tests/_parity.py (32 mel frames / 2048 samples per window)."""
import numpy as np
import pytest
import torch

from _parity import check_localised, dit_v3_chunk_case, rel_rms
from gsv import synthetic as S
from oracle import cfm_oracle, vocoder_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEL_WIN, WAV_WIN = 32, 2048
# worst window / median window: measured 1.02 - 1.07 on the MI355X over every comparison below (each test's docstring gives
# its own); 3 leaves room for run-to-run noise, and one window with more than 3x the median error fails
LOC_FACTOR = 3.0


def _cfm(cfg, sd, dtype):
    from gsv.f5_tts.model.backbones.dit import DiT
    from gsv.module.models import CFM
    dit = DiT(dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], dim_head=cfg["dim_head"], ff_mult=cfg["ff_mult"],
              mel_dim=cfg["mel_dim"], text_dim=cfg["text_dim"], conv_layers=cfg["conv_layers"], device=DEV, dtype=dtype)
    dit.load_state_dict({"cfm.estimator." + k: v for k, v in sd.items()})
    return CFM(cfg["mel_dim"], dit)


def _vocoder(cfg, sd, dtype):
    if cfg["kind"] == "hifigan":
        from gsv.module.models import Generator
        m = Generator(initial_channel=cfg["initial_channel"], resblock=cfg["resblock"],
                      resblock_kernel_sizes=cfg["resblock_kernel_sizes"],
                      resblock_dilation_sizes=cfg["resblock_dilation_sizes"], upsample_rates=cfg["upsample_rates"],
                      upsample_initial_channel=cfg["upsample_initial_channel"],
                      upsample_kernel_sizes=cfg["upsample_kernel_sizes"], gin_channels=0, is_bias=True, device=DEV, dtype=dtype)
    else:
        from gsv.BigVGAN.bigvgan import BigVGAN
        m = BigVGAN({k: v for k, v in cfg.items() if k != "kind"}, device=DEV, dtype=dtype)
    m.load_state_dict(sd)
    return m


def _check_fp16_mel(out, ref, Tp, label):
    """the fp16 DiT bar: prompt frames exactly 0, finite, relative RMS <= 3 % and max-abs <= 0.15, localised over the
    generated frames"""
    assert out.shape == ref.shape and Tp > 0
    assert float(out[..., :Tp].abs().max()) == 0.0
    assert torch.isfinite(out).all()
    err = (out - ref).abs().max().item()
    rel = rel_rms(out, ref)
    print(f"[parity] {label}: max-abs error {err:.2e}, relative rms {rel * 100:.2f} % (mel rms {ref.pow(2).mean().sqrt():.3f})")
    assert rel <= 0.03 and err <= 0.15
    check_localised(out[..., Tp:].numpy(), ref[..., Tp:].numpy(), MEL_WIN, 0.03, LOC_FACTOR, label)


def test_fp16_dit_full_depth_at_chunk_length_vs_oracle():
    """A. The production DiT in fp16 at one chunk: 1024 x 22 blocks, T = 934, Tp = 468, 2 Euler steps, the same weights,
    inputs and (shared) oracle output as test_cfm_gpu.py::test_cfm_full_depth_at_chunk_length_vs_oracle.  Measured: max-abs
    5.4e-3, relative rms 0.09 %, worst / median window 1.03."""
    cfg, sd, mu, prompt, noise, steps, ref = dit_v3_chunk_case()
    out = _cfm(cfg, sd, torch.float16).inference(mu.to(DEV), None, prompt.to(DEV), steps, noise=noise).float().cpu()
    assert out.shape == (1, 100, 934)
    _check_fp16_mel(out, ref, prompt.shape[-1], "fp16 depth-22 DiT, T=934, 2 steps")


def test_fp16_dit_full_depth_batched_chunks_distinct_rows():
    """B. The batched-chunk call (using_vocoder_synthesis_batched_infer at the bench's B = 8): 8 x 934 rows, each chunk with
    its own mu and noise and one prompt broadcast over the batch.  Every row equals a B = 1 run of the same chunk within the
    fp16 bar (the two runs take different GEMM kernels), rows 0 and 7 match the oracle within the fp16 DiT bar, and the
    rows differ from one another (a row-offset bug that repeats one chunk fails).  Measured: rows vs B = 1 max-abs <= 3.8e-3,
    0.055 % relative rms, worst / median window <= 1.06; rows 0 and 7 vs the oracle 6.0e-3 / 0.09 %."""
    cfg, sd, _, prompt, _, steps, _ = dit_v3_chunk_case()
    B, T, Tp = 8, 934, prompt.shape[-1]
    mu = torch.cat([S.hash_symmetric("b8_mu", (1, T, cfg["text_dim"]), 1.0, 100 + b) for b in range(B)])
    noise = torch.cat([S.hash_normal("b8_noise", (1, cfg["mel_dim"], T), 200 + b) for b in range(B)])
    cfm = _cfm(cfg, sd, torch.float16)
    out = cfm.inference(mu.to(DEV), None, prompt.to(DEV), steps, noise=noise).float().cpu()
    assert out.shape == (B, 100, T) and torch.isfinite(out).all()
    assert float(out[..., :Tp].abs().max()) == 0.0
    for b in range(B):
        one = cfm.inference(mu[b:b + 1].to(DEV), None, prompt.to(DEV), steps, noise=noise[b:b + 1]).float().cpu()
        err = (out[b:b + 1] - one).abs().max().item()
        rel = rel_rms(out[b:b + 1, :, Tp:], one[..., Tp:])
        print(f"[parity] fp16 DiT B=8 row {b} vs its B=1 run: max-abs {err:.2e}, relative rms {rel * 100:.3f} %")
        assert rel <= 0.03 and err <= 0.15
        check_localised(out[b:b + 1, :, Tp:].numpy(), one[..., Tp:].numpy(), MEL_WIN, 0.03, LOC_FACTOR, f"B=8 row {b} vs B=1")
    for i in range(B):
        for j in range(i + 1, B):
            assert rel_rms(out[i, :, Tp:], out[j, :, Tp:]) > 0.3, f"rows {i} and {j} of the batch are (nearly) the same"
    torch.set_num_threads(8)
    pick = [0, B - 1]
    ref = cfm_oracle.cfm_inference(sd, cfg, mu[pick], prompt, steps, noise[pick].clone())
    for k, b in enumerate(pick):
        _check_fp16_mel(out[b:b + 1], ref[k:k + 1], Tp, f"fp16 depth-22 DiT, B=8 row {b} vs oracle")


def test_dit_32_euler_steps_vs_oracle():
    """C. The bench's N = 32 Euler steps (the modulation table is indexed step by step) on the reduced DiT at T = 934 with a
    300-frame prompt: fp32 engine max-abs <= 2e-3, fp16 engine within the fp16 DiT bar.  Measured: fp32 2.4e-6; fp16 2.7e-3,
    0.04 % relative rms, worst / median window 1.05."""
    cfg = S.small_dit_config()
    sd = S.make_dit_state_dict(cfg, seed=21)
    T, Tp, N = 934, 300, 32
    mu = S.hash_symmetric("n32_mu", (1, T, cfg["text_dim"]), 1.0, 1)
    prompt = S.hash_symmetric("n32_prompt", (1, cfg["mel_dim"], Tp), 1.0, 2)
    noise = S.hash_normal("n32_noise", (1, cfg["mel_dim"], T), 3)
    torch.set_num_threads(8)
    ref = cfm_oracle.cfm_inference(sd, cfg, mu, prompt, N, noise.clone())
    out = _cfm(cfg, sd, torch.float32).inference(mu.to(DEV), None, prompt.to(DEV), N, noise=noise).cpu()
    err = (out - ref).abs().max().item()
    print(f"[parity] fp32 reduced DiT, T=934, 32 steps: max-abs error {err:.2e} (mel rms {ref.pow(2).mean().sqrt():.3f})")
    assert out.shape == ref.shape and err <= 2e-3
    assert float(out[..., :Tp].abs().max()) == 0.0
    o16 = _cfm(cfg, sd, torch.float16).inference(mu.to(DEV), None, prompt.to(DEV), N, noise=noise).float().cpu()
    _check_fp16_mel(o16, ref, Tp, "fp16 reduced DiT, T=934, 32 steps")



def test_dit_rotary_at_late_positions_vs_oracle():
    """F. The rotary embedding at positions up to 933 (applied inside the flash / V^T launch in fp16, by its own kernel in
    fp32).  It rotates only the first 64 channels of the projections (head 0), and with the synthetic weights attention is
    close to uniform, so a rotary error moves the output little: with those weights, dropping the query rotation from row
    512 on changes the mel by 0.6 % (oracle run on the host), inside the fp16 bar.  Here the query and key weights are
    scaled by 3, which makes attention sharp as in a trained model: the same fault then moves the mel by 6.5 % overall and
    by 7.6 - 8.3 % in the windows past row 544.  Reduced DiT (2 heads: rotary on half of them), T = 934, Tp = 300, 2 Euler steps:
    fp32 engine max-abs <= 2e-3, fp16 engine within the fp16 DiT bar.  Measured: fp32 2.1e-5; fp16 4.0e-3, 0.06 % relative
    rms, worst / median window 1.05; with the query rotation dropped from row 512 on, the fp16 run fails at 6.5 %."""
    cfg = S.small_dit_config()
    sd = S.make_dit_state_dict(cfg, seed=21)
    for i in range(cfg["depth"]):
        for n in ("to_q", "to_k"):
            sd[f"transformer_blocks.{i}.attn.{n}.weight"] = sd[f"transformer_blocks.{i}.attn.{n}.weight"] * 3.0
    T, Tp, N = 934, 300, 2
    mu = S.hash_symmetric("rope_mu", (1, T, cfg["text_dim"]), 1.0, 1)
    prompt = S.hash_symmetric("rope_prompt", (1, cfg["mel_dim"], Tp), 1.0, 2)
    noise = S.hash_normal("rope_noise", (1, cfg["mel_dim"], T), 3)
    torch.set_num_threads(8)
    ref = cfm_oracle.cfm_inference(sd, cfg, mu, prompt, N, noise.clone())
    out = _cfm(cfg, sd, torch.float32).inference(mu.to(DEV), None, prompt.to(DEV), N, noise=noise).cpu()
    err = (out - ref).abs().max().item()
    print(f"[parity] fp32 reduced DiT, sharp attention, T=934: max-abs error {err:.2e}")
    assert out.shape == ref.shape and err <= 2e-3
    o16 = _cfm(cfg, sd, torch.float16).inference(mu.to(DEV), None, prompt.to(DEV), N, noise=noise).float().cpu()
    _check_fp16_mel(o16, ref, Tp, "fp16 reduced DiT, sharp attention, T=934")

def _vocoder_at_length(cfg, seed, F, label):
    sd = S.make_vocoder_state_dict(cfg, seed=seed)
    mel = S.hash_symmetric("bench_voc_mel", (1, 100, F), 7.0, seed) - 5.0      # the bench's clamp range [-12, 2]
    torch.set_num_threads(8)
    ref = (vocoder_oracle.bigvgan if cfg["kind"] == "bigvgan" else vocoder_oracle.hifigan)(sd, cfg, mel)
    out = _vocoder(cfg, sd, torch.float32)(mel.to(DEV)).float().cpu()
    assert out.shape == ref.shape == (1, 1, F * int(np.prod(cfg["upsample_rates"])))
    err = (out - ref).abs().max().item()
    print(f"[parity] fp32 {label}, F={F}: max-abs error {err:.2e} (waveform rms {ref.pow(2).mean().sqrt():.3f})")
    assert err <= 2e-4
    o16 = _vocoder(cfg, sd, torch.float16)(mel.to(DEV)).float().cpu()
    assert o16.shape == ref.shape and torch.isfinite(o16).all()
    err = (o16 - ref).abs().max().item()
    rel = rel_rms(o16, ref)
    print(f"[parity] fp16 {label}, F={F}: max-abs error {err:.2e}, relative rms {rel * 100:.2f} %")
    assert err <= 3e-2 and rel <= 0.05
    check_localised(o16.numpy(), ref.numpy(), WAV_WIN, 0.05, LOC_FACTOR, f"fp16 {label}")


def test_bigvgan_v2_full_config_at_bench_length_vs_oracle():
    """D. BigVGAN-v2 (24 kHz, 256x) on the bench's 466-frame mel: stages of 1864 ... 119 296 samples, i.e. many anti-alias
    tiles per sequence.  Measured: fp32 9.6e-6; fp16 4.4e-3, 0.19 % relative rms, worst / median window 1.07."""
    _vocoder_at_length(dict(S.BIGVGAN_V2_24K_CONFIG), 31, 466, "BigVGAN-v2")


def test_hifigan_v4_full_config_at_length_vs_oracle():
    """E. The v4 HiFi-GAN vocoder at F = 300 (>= 274, so the 128-channel stage reaches `conv_wide`): stages of 3000 ...
    144 000 samples through `conv_wide`, the persistent 64-channel narrow conv, the 32 / 16-channel ResBlock pairs and the
    persistent `conv_narrow<16>` conv_post.  Measured: fp32 1.9e-6; fp16 1.7e-3, 0.11 % relative rms, worst / median window
    1.05."""
    _vocoder_at_length(dict(S.HIFIGAN_V4_CONFIG), 32, 300, "v4 HiFi-GAN")
