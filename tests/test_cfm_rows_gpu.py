"""GPU: gsv_cfm_inference_rows / CFM.inference_rows -- B rows of a common length, each with its own prompt mel, prompt length
and noise key, in one flow-matching pass -- against cfm_oracle run on each row alone, against gsv_cfm_inference, and for the
properties a shared pass over several voices relies on (row independence, determinism, bounds, argument errors)."""
import ctypes as C

import pytest
import torch

from _parity import check_localised, dit_v3_chunk_case, rel_rms
from gsv import synthetic as S
from oracle import cfm_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = 0x9E3779B97F4A7C15
MASK = 0xFFFFFFFFFFFFFFFF
MEL_WIN, LOC_FACTOR = 32, 3.0          # the window check of test_v3_bench_shapes_gpu.py


def _cfm(cfg, sd, dtype):
    from gsv.f5_tts.model.backbones.dit import DiT
    from gsv.module.models import CFM
    dit = DiT(dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], dim_head=cfg["dim_head"], ff_mult=cfg["ff_mult"],
              mel_dim=cfg["mel_dim"], text_dim=cfg["text_dim"], conv_layers=cfg["conv_layers"], device=DEV, dtype=dtype)
    dit.load_state_dict({"cfm.estimator." + k: v for k, v in sd.items()})
    return CFM(cfg["mel_dim"], dit)


def _rows(cfg, T, tps, tag):
    B = len(tps)
    mu = torch.cat([S.hash_symmetric(f"{tag}_mu", (1, T, cfg["text_dim"]), 1.0, 100 + b) for b in range(B)])
    noise = torch.cat([S.hash_normal(f"{tag}_noise", (1, cfg["mel_dim"], T), 200 + b) for b in range(B)])
    prompts = [S.hash_symmetric(f"{tag}_prompt", (1, cfg["mel_dim"], tp), 1.0, 300 + b) for b, tp in enumerate(tps)]
    return mu, prompts, noise


def _small():
    cfg = S.small_dit_config()
    T = 40
    tps = [0, 1, 17, T - 1, T]
    return cfg, S.make_dit_state_dict(cfg, seed=5), T, tps, 3


def _oracle_rows(sd, cfg, mu, prompts, steps, noise):
    """every row through the oracle on its own: B = 1, its own prompt"""
    return [cfm_oracle.cfm_inference(sd, cfg, mu[b:b + 1], p, steps, noise[b:b + 1].clone()) for b, p in enumerate(prompts)]


def _check_fp16_row(out, ref, Tp, label):
    """the fp16 DiT bar of test_v3_bench_shapes_gpu.py for one row: prompt frames exactly 0, finite, relative RMS <= 3 %,
    max-abs <= 0.15, and the per-window check over the generated frames"""
    assert out.shape == ref.shape and torch.isfinite(out).all()
    assert Tp == 0 or float(out[..., :Tp].abs().max()) == 0.0
    if Tp == out.shape[-1]:
        assert float(ref.abs().max()) == 0.0
        return
    err, rel = (out - ref).abs().max().item(), rel_rms(out, ref)
    print(f"[parity] {label}: max-abs error {err:.2e}, relative rms {rel * 100:.3f} %")
    assert rel <= 0.03 and err <= 0.15
    check_localised(out[..., Tp:].numpy(), ref[..., Tp:].numpy(), MEL_WIN, 0.03, LOC_FACTOR, label)


def test_fp32_rows_match_the_oracle_row_by_row():
    """fp32, 5 rows with Tp = 0, 1, 17, T - 1, T and different prompts: every row within the fp32 CFM bar (2e-3 max-abs,
    test_cfm_gpu.py) of the oracle run on that row alone; its first Tp frames exactly zero."""
    cfg, sd, T, tps, steps = _small()
    mu, prompts, noise = _rows(cfg, T, tps, "rows")
    out = _cfm(cfg, sd, torch.float32).inference_rows(mu.to(DEV), [p.to(DEV) for p in prompts], steps, noise=noise).cpu()
    assert out.shape == (len(tps), cfg["mel_dim"], T)
    for b, ref in enumerate(_oracle_rows(sd, cfg, mu, prompts, steps, noise)):
        err = (out[b:b + 1] - ref).abs().max().item()
        print(f"[parity] fp32 row {b} (Tp = {tps[b]}): max-abs error {err:.2e}")
        assert err <= 2e-3
        assert tps[b] == 0 or float(out[b, :, :tps[b]].abs().max()) == 0.0
    assert float(out[4].abs().max()) == 0.0 and float(out[3, :, -1].abs().max()) > 0.0


def test_fp16_rows_match_the_oracle_row_by_row():
    """the same rows through the fp16 engine (the fused attention with the row as a grid dimension): the fp16 DiT bar"""
    cfg, sd, T, tps, steps = _small()
    mu, prompts, noise = _rows(cfg, T, tps, "rows")
    out = _cfm(cfg, sd, torch.float16).inference_rows(mu.to(DEV), [p.to(DEV) for p in prompts], steps, noise=noise).float().cpu()
    for b, ref in enumerate(_oracle_rows(sd, cfg, mu, prompts, steps, noise)):
        _check_fp16_row(out[b:b + 1], ref, tps[b], f"fp16 row {b} (Tp = {tps[b]})")


def test_fp16_production_dit_three_voices_at_chunk_length():
    """DiT 1024 x 22, T = 934, fp16, 2 Euler steps: row 0 is the case of test_v3_bench_shapes_gpu.py test A (Tp = 468), row 1
    another chunk behind a 300-frame prompt, row 2 one without a prompt.  Each within the fp16 DiT bar of the oracle run on it
    alone.  Three rows of 16 heads are 48 (row, head) pairs, 6 to an XCD: the runs of XCDs 2 and 5 hold heads of two rows, which
    an even row count never gives.  (The grid is 15 x 16 x B workgroups, a multiple of 8 for every B, so the uneven-run branch
    of xcd_virtual_id is taken by the small configurations only.)"""
    cfg, sd, mu0, prompt0, noise0, steps, ref0 = dit_v3_chunk_case()
    T, tps = 934, [300, 0]
    mu1, p1, nz1 = _rows(cfg, T, tps, "rows1024")
    torch.set_num_threads(8)
    ref1 = _oracle_rows(sd, cfg, mu1, p1, steps, nz1)
    out = _cfm(cfg, sd, torch.float16).inference_rows(torch.cat([mu0, mu1]).to(DEV), [prompt0.to(DEV)] + [p.to(DEV) for p in p1], steps,
                                                      noise=torch.cat([noise0, nz1])).float().cpu()
    _check_fp16_row(out[0:1], ref0, 468, "fp16 depth-22 DiT rows, row 0 (Tp = 468)")
    for b, tp in enumerate(tps):
        _check_fp16_row(out[b + 1:b + 2], ref1[b], tp, f"fp16 depth-22 DiT rows, row {b + 1} (Tp = {tp})")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_row_seeds_reproduce_the_uniform_entry_bit_for_bit(dtype):
    """Without injected noise: row b of a rows call with seed s + 0x9E37...15 * b against row b of gsv_cfm_inference with seed
    s and the same uniform Tp.  BIT-EQUAL: gsv_cfm_inference builds a uniform row table and runs the very same kernels, so
    there is one code path and the two calls issue identical launches."""
    cfg, sd, T, _, steps = _small()
    B, Tp, s = 4, 11, 1234567
    mu, _, _ = _rows(cfg, T, [Tp] * B, "seeded")
    prompt = S.hash_symmetric("seeded_prompt", (B, cfg["mel_dim"], Tp), 1.0, 9)
    cfm = _cfm(cfg, sd, dtype)
    old = cfm.inference(mu.to(DEV), None, prompt.to(DEV), steps, seed=s)
    new = cfm.inference_rows(mu.to(DEV), [prompt[b:b + 1].to(DEV) for b in range(B)], steps,
                             seeds=[(s + GOLDEN * b) & MASK for b in range(B)])
    assert torch.isfinite(new).all() and float(new[..., Tp:].abs().max()) > 0
    assert torch.equal(old, new)
    other = cfm.inference_rows(mu.to(DEV), [prompt[b:b + 1].to(DEV) for b in range(B)], steps, seeds=[s + 1 + b for b in range(B)])
    assert not torch.equal(other, new)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_rows_are_independent_and_calls_repeat(dtype):
    """swapping the prompts of two rows changes those two rows and no other, bit for bit; a second identical call is
    bit-identical"""
    cfg, sd, T, tps, steps = _small()
    mu, prompts, noise = _rows(cfg, T, tps, "rows")
    cfm = _cfm(cfg, sd, dtype)
    dev = [p.to(DEV) for p in prompts]
    a = cfm.inference_rows(mu.to(DEV), dev, steps, noise=noise)
    again = cfm.inference_rows(mu.to(DEV), dev, steps, noise=noise)
    assert torch.equal(a, again)
    sw = list(dev)
    sw[1], sw[2] = dev[2], dev[1]                      # Tp = 1 and Tp = 17
    b = cfm.inference_rows(mu.to(DEV), sw, steps, noise=noise)
    for r in (0, 3, 4):
        assert torch.equal(a[r], b[r]), f"row {r} changed with the prompts of rows 1 and 2"
    assert not torch.equal(a[1], b[1]) and not torch.equal(a[2], b[2])
    assert float(b[1, :, :17].abs().max()) == 0.0 and float(b[2, :, 1:].abs().max()) > 0.0


def _raw(cfm, mu, ptrs, tps, B, T, steps, noise, seeds, out):
    from gsv import _lib
    dit = cfm.estimator
    rc = _lib.lib().gsv_cfm_inference_rows(dit._h, mu.data_ptr(), (C.c_void_p * len(ptrs))(*ptrs) if ptrs is not None else None,
                                           (C.c_int * len(tps))(*tps), B, T, steps, noise.data_ptr() if noise is not None else None,
                                           (C.c_uint64 * len(seeds))(*seeds) if seeds is not None else None, 1.0, out.data_ptr(),
                                           C.c_void_p(dit.stream.cuda_stream))
    dit.stream.synchronize()
    return rc


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_output_bounds_and_bad_arguments(dtype):
    """NaN sentinels behind `out` stay intact; Tp_b > T, a null prompt with Tp_b > 0, B = 0 and neither noise nor seeds
    return an error and write nothing"""
    cfg, sd, T, tps, steps = _small()
    B, md = len(tps), cfg["mel_dim"]
    mu, prompts, noise = _rows(cfg, T, tps, "rows")
    cfm = _cfm(cfg, sd, dtype)
    with torch.cuda.device(DEV):
        m = mu.to(DEV).contiguous()
        nz = noise.to(DEV).contiguous()
        ps = [p.to(DEV).contiguous() for p in prompts]
        ptrs = [p.data_ptr() if p.shape[2] else None for p in ps]
        n, guard = B * md * T, 4096
        out = torch.full((n + guard,), float("nan"), device=DEV)
        torch.cuda.synchronize()
        assert _raw(cfm, m, ptrs, tps, B, T, steps, nz, None, out) == 0
        assert torch.isfinite(out[:n]).all() and torch.isnan(out[n:]).all()
        want = cfm.inference_rows(mu.to(DEV), ps, steps, noise=noise).float().reshape(-1)
        assert torch.equal(out[:n], want)
        # with seeds instead of noise
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        assert _raw(cfm, m, ptrs, tps, B, T, steps, None, list(range(7, 7 + B)), out) == 0
        assert torch.isfinite(out[:n]).all() and torch.isnan(out[n:]).all()
        # errors: nothing is launched, so nothing is written
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        bad_tp = list(tps)
        bad_tp[2] = T + 1
        assert _raw(cfm, m, ptrs, bad_tp, B, T, steps, nz, None, out) != 0
        null_p = list(ptrs)
        null_p[2] = None
        assert _raw(cfm, m, null_p, tps, B, T, steps, nz, None, out) != 0
        assert _raw(cfm, m, None, tps, B, T, steps, nz, None, out) != 0
        assert _raw(cfm, m, ptrs, tps, 0, T, steps, nz, None, out) != 0
        assert _raw(cfm, m, ptrs, tps, B, T, steps, None, None, out) != 0
        neg = list(tps)
        neg[0] = -1
        assert _raw(cfm, m, ptrs, neg, B, T, steps, nz, None, out) != 0
        torch.cuda.synchronize()
        assert torch.isnan(out).all()
    # the host mirror raises in the style of CFM.inference
    with pytest.raises(ValueError):
        cfm.inference_rows(mu.to(DEV), ps, steps)                                   # neither noise nor seeds
    with pytest.raises(ValueError):
        cfm.inference_rows(mu.to(DEV), ps[:-1], steps, noise=noise)                 # one prompt per row
    with pytest.raises(ValueError):
        cfm.inference_rows(mu[:, :30].to(DEV), ps, steps, seeds=[1] * B)            # Tp_b > T
    with pytest.raises(ValueError):
        cfm.inference_rows(mu[:0].to(DEV), [], steps, seeds=[])                     # B = 0
    with pytest.raises(ValueError):
        cfm.inference_rows(mu.to(DEV), ps, steps, seeds=[1, 2])
