"""GPU: classifier-free guidance in the flow-matching decoder -- gsv_cfm_inference_guided / CFM.inference_guided and
CFM.inference_rows(..., inference_cfg_rate=r): every request row and its unconditioned twin in ONE DiT pass over 2 B rows -- against tests/_cfg_ref.py
(the reference's guided loop restated, pinned by test_cfm_cfg_oracle.py) run on each row alone, against the unguided entries
at and below the rate threshold, and for the properties a shared pass relies on (row independence, determinism, noise keys,
bounds, argument errors).  Rows, shapes and bars are those of test_cfm_rows_gpu.py."""
import ctypes as C
import functools

import pytest
import torch

import _cfg_ref
from _parity import dit_v3_chunk_case
from gsv import synthetic as S
from test_cfm_rows_gpu import DEV, GOLDEN, MASK, _cfm, _check_fp16_row, _rows, _small

pytestmark = pytest.mark.gpu
RATES = _cfg_ref.RATES


@functools.lru_cache(maxsize=None)
def _ref_rows(rate):
    """every row of the small case through the helper on its own (B = 1, its own prompt), once per session and rate"""
    cfg, sd, T, tps, steps = _small()
    mu, prompts, noise = _rows(cfg, T, tps, "rows")
    return tuple(_cfg_ref.cfm_inference_cfg(sd, cfg, mu[b:b + 1], p, steps, noise[b:b + 1].clone(), rate) for b, p in enumerate(prompts))


def _guided(dtype, rate, **kw):
    cfg, sd, T, tps, steps = _small()
    mu, prompts, noise = _rows(cfg, T, tps, "rows")
    return _cfm(cfg, sd, dtype).inference_rows(mu.to(DEV), [p.to(DEV) for p in prompts], steps, noise=noise, inference_cfg_rate=rate,
                                               **kw).float().cpu()


@pytest.mark.parametrize("rate", RATES)
def test_fp32_guided_rows_match_the_helper_row_by_row(rate):
    """fp32, 5 rows with Tp = 0, 1, 17, T - 1, T: every row within the fp32 CFM bar (2e-3 max-abs) of the helper run on that
    row alone; its first Tp frames exactly zero."""
    cfg, sd, T, tps, steps = _small()
    out = _guided(torch.float32, rate)
    assert out.shape == (len(tps), cfg["mel_dim"], T)
    for b, ref in enumerate(_ref_rows(rate)):
        err = (out[b:b + 1] - ref).abs().max().item()
        print(f"[parity] fp32 guided r = {rate} row {b} (Tp = {tps[b]}): max-abs error {err:.2e}")
        assert err <= 2e-3
        assert tps[b] == 0 or float(out[b, :, :tps[b]].abs().max()) == 0.0
    assert float(out[4].abs().max()) == 0.0 and float(out[3, :, -1].abs().max()) > 0.0


@pytest.mark.parametrize("rate", RATES)
def test_fp16_guided_rows_match_the_helper_row_by_row(rate):
    """the same rows through the fp16 engine (10 rows of the fused attention): the fp16 DiT bar -- relative rms <= 3 %,
    max-abs <= 0.15, the per-window check"""
    cfg, sd, T, tps, steps = _small()
    out = _guided(torch.float16, rate)
    for b, ref in enumerate(_ref_rows(rate)):
        _check_fp16_row(out[b:b + 1], ref, tps[b], f"fp16 guided r = {rate} row {b} (Tp = {tps[b]})")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_rate_at_or_below_the_threshold_is_todays_pass_bit_for_bit(dtype):
    """guidance is active iff rate > 1e-5 (models.py:1063): 0, 1e-6, exactly 1e-5 and a negative rate issue the unguided
    launches, with injected noise and with seeds"""
    cfg, sd, T, tps, steps = _small()
    mu, prompts, noise = _rows(cfg, T, tps, "rows")
    cfm = _cfm(cfg, sd, dtype)
    dev = [p.to(DEV) for p in prompts]
    seeds = list(range(21, 21 + len(tps)))
    plain = cfm.inference_rows(mu.to(DEV), dev, steps, noise=noise)
    seeded = cfm.inference_rows(mu.to(DEV), dev, steps, seeds=seeds)
    for rate in (0, 1e-6, 1e-5, -2.0):
        assert torch.equal(cfm.inference_rows(mu.to(DEV), dev, steps, noise=noise, inference_cfg_rate=rate), plain), rate
        assert torch.equal(cfm.inference_rows(mu.to(DEV), dev, steps, seeds=seeds, inference_cfg_rate=rate), seeded), rate
    old = cfm.inference(mu.to(DEV), None, dev[2].expand(len(tps), -1, -1), steps, seed=5)
    assert torch.equal(cfm.inference_guided(mu.to(DEV), None, dev[2].expand(len(tps), -1, -1), steps, seed=5, inference_cfg_rate=1e-6), old)
    assert torch.equal(cfm.inference(mu.to(DEV), None, dev[2].expand(len(tps), -1, -1), steps, seed=5, inference_cfg_rate=1e-6), old)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_uniform_entry_is_the_rows_entry_with_its_seeds(dtype):
    """CFM.inference_guided(inference_cfg_rate=0.7, seed=s) -- the uniform, guided entry -- is bit-equal to inference_rows(seeds=[s + GOLDEN * b], same rate), with a
    per-row prompt and with one prompt broadcast over the batch"""
    cfg, sd, T, _, steps = _small()
    B, Tp, s = 4, 11, 1234567
    mu, _, _ = _rows(cfg, T, [Tp] * B, "seeded")
    prompt = S.hash_symmetric("seeded_prompt", (B, cfg["mel_dim"], Tp), 1.0, 9).to(DEV)
    cfm = _cfm(cfg, sd, dtype)
    seeds = [(s + GOLDEN * b) & MASK for b in range(B)]
    uni = cfm.inference_guided(mu.to(DEV), None, prompt, steps, inference_cfg_rate=0.7, seed=s)
    rows = cfm.inference_rows(mu.to(DEV), [prompt[b:b + 1] for b in range(B)], steps, seeds=seeds, inference_cfg_rate=0.7)
    assert torch.isfinite(uni).all() and float(uni[..., Tp:].abs().max()) > 0 and float(uni[..., :Tp].abs().max()) == 0
    assert torch.equal(uni, rows)
    one = cfm.inference_guided(mu.to(DEV), None, prompt[:1], steps, inference_cfg_rate=0.7, seed=s)
    assert torch.equal(one, cfm.inference_rows(mu.to(DEV), [prompt[:1]] * B, steps, seeds=seeds, inference_cfg_rate=0.7))
    assert not torch.equal(uni, cfm.inference(mu.to(DEV), None, prompt, steps, seed=s)), "the rate changed nothing"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_guided_rows_are_independent_and_calls_repeat(dtype):
    """The standard of test_rows_are_independent_and_calls_repeat, guided: swapping the prompts of two rows changes those two
    rows and no other, bit for bit (a twin reads its own row's x and nobody's prompt); a second identical call is
    bit-identical.  A row alone (2 DiT rows) equals the same row in the batch of 5 (10 DiT rows), bit for bit: every GEMM
    row, attention (row, head) pair and time-axis kernel does the arithmetic it does alone."""
    cfg, sd, T, tps, steps = _small()
    mu, prompts, noise = _rows(cfg, T, tps, "rows")
    cfm = _cfm(cfg, sd, dtype)
    dev = [p.to(DEV) for p in prompts]
    a = cfm.inference_rows(mu.to(DEV), dev, steps, noise=noise, inference_cfg_rate=0.7)
    again = cfm.inference_rows(mu.to(DEV), dev, steps, noise=noise, inference_cfg_rate=0.7)
    assert torch.equal(a, again)
    sw = list(dev)
    sw[1], sw[2] = dev[2], dev[1]                      # Tp = 1 and Tp = 17
    b = cfm.inference_rows(mu.to(DEV), sw, steps, noise=noise, inference_cfg_rate=0.7)
    for r in (0, 3, 4):
        assert torch.equal(a[r], b[r]), f"row {r} changed with the prompts of rows 1 and 2"
    assert not torch.equal(a[1], b[1]) and not torch.equal(a[2], b[2])
    assert float(b[1, :, :17].abs().max()) == 0.0 and float(b[2, :, 1:].abs().max()) > 0.0
    for r in (0, 2, 3):
        alone = cfm.inference_rows(mu[r:r + 1].to(DEV), dev[r:r + 1], steps, noise=noise[r:r + 1], inference_cfg_rate=0.7)
        err = (alone.float() - a[r:r + 1].float()).abs().max().item()
        print(f"[parity] {dtype} guided row {r} alone vs in the batch of 5: max-abs {err:.2e}")
        assert torch.equal(alone, a[r:r + 1]), f"row {r} alone differs from the same row in the batch by {err:.2e}"


def test_rate_is_honoured():
    """guided and unguided outputs of the same rows differ by more than 0.1 max-abs on the generated frames (the reference's
    own difference at r = 0.7 is 1.4), and r = 0.7 differs from r = 2.0"""
    cfg, sd, T, tps, steps = _small()
    plain, g07, g20 = _guided(torch.float32, 0), _guided(torch.float32, 0.7), _guided(torch.float32, 2.0)
    for b, tp in enumerate(tps):
        if tp == T:
            continue
        d = (g07[b, :, tp:] - plain[b, :, tp:]).abs().max().item()
        print(f"guided (0.7) - unguided, row {b}: max-abs {d:.2f}")
        assert d > 0.1
        assert (g20[b, :, tp:] - g07[b, :, tp:]).abs().max().item() > 0.1


def test_device_noise_is_the_unguided_draw():
    """noise=None: a guided call draws what the unguided call with the same seeds draws (the twins draw nothing: the Euler
    state has B rows).  Checked just above the threshold, r = 2e-5, where guidance is active but moves the exact result by
    2e-5 x d(out)/d(rate) ~ 2e-5 x 2 (the reference moves 1.4 for 0.7): both engine outputs are within the fp32 bar 2e-3 of
    their exact results, so they are within 2 x 2e-3 + 1e-4 of each other if and only if the draw is the same one -- another
    draw differs by O(1).  Also finite, reproducible, and keyed by the seeds."""
    cfg, sd, T, tps, steps = _small()
    mu, prompts, _ = _rows(cfg, T, tps, "rows")
    cfm = _cfm(cfg, sd, torch.float32)
    dev = [p.to(DEV) for p in prompts]
    seeds = [(77 + GOLDEN * b) & MASK for b in range(len(tps))]
    plain = cfm.inference_rows(mu.to(DEV), dev, steps, seeds=seeds)
    barely = cfm.inference_rows(mu.to(DEV), dev, steps, seeds=seeds, inference_cfg_rate=2e-5)
    err = (barely - plain).abs().max().item()
    print(f"guided at r = 2e-5 vs unguided, same seeds: max-abs {err:.2e}")
    assert err <= 2 * 2e-3 + 1e-4
    g = cfm.inference_rows(mu.to(DEV), dev, steps, seeds=seeds, inference_cfg_rate=0.7)
    assert torch.isfinite(g).all() and float(g[0].abs().max()) > 0
    assert torch.equal(g, cfm.inference_rows(mu.to(DEV), dev, steps, seeds=seeds, inference_cfg_rate=0.7))
    other = cfm.inference_rows(mu.to(DEV), dev, steps, seeds=[s + 1 for s in seeds], inference_cfg_rate=0.7)
    assert not torch.equal(other[0], g[0])


def _raw(cfm, mu, ptrs, tps, B, T, steps, noise, seeds, rate, out):
    from gsv import _lib
    dit = cfm.estimator
    rc = _lib.lib().gsv_cfm_inference_guided(dit._h, mu.data_ptr(), (C.c_void_p * len(ptrs))(*ptrs) if ptrs is not None else None,
                                             (C.c_int * len(tps))(*tps), B, T, steps, noise.data_ptr() if noise is not None else None,
                                             (C.c_uint64 * len(seeds))(*seeds) if seeds is not None else None, 1.0, rate,
                                             out.data_ptr(), C.c_void_p(dit.stream.cuda_stream))
    dit.stream.synchronize()
    return rc


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_output_bounds_and_bad_arguments(dtype):
    """NaN sentinels behind `out` stay intact after a guided call; a non-finite rate, more than 65535 DiT rows, Tp_b > T, a
    null prompt with Tp_b > 0, B = 0 and neither noise nor seeds return an error and write nothing.  The host mirror raises
    ValueError for a non-finite rate; a positive one runs (through inference_guided: no NotImplementedError there)."""
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
        assert _raw(cfm, m, ptrs, tps, B, T, steps, nz, None, 0.7, out) == 0
        assert torch.isfinite(out[:n]).all() and torch.isnan(out[n:]).all()
        want = cfm.inference_rows(mu.to(DEV), ps, steps, noise=noise, inference_cfg_rate=0.7).float().reshape(-1)
        assert torch.equal(out[:n], want)
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        assert _raw(cfm, m, ptrs, tps, B, T, steps, None, list(range(7, 7 + B)), 0.7, out) == 0
        assert torch.isfinite(out[:n]).all() and torch.isnan(out[n:]).all()
        # errors: nothing is launched, so nothing is written
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        for bad in (float("nan"), float("inf"), float("-inf")):
            assert _raw(cfm, m, ptrs, tps, B, T, steps, nz, None, bad, out) != 0
        many = 32768                                   # 2 * 32768 rows exceed the grid; unguided, 32768 rows would be accepted
        assert _raw(cfm, m, [None] * many, [0] * many, many, T, steps, nz, None, 0.7, out) != 0
        bad_tp = list(tps)
        bad_tp[2] = T + 1
        assert _raw(cfm, m, ptrs, bad_tp, B, T, steps, nz, None, 0.7, out) != 0
        null_p = list(ptrs)
        null_p[2] = None
        assert _raw(cfm, m, null_p, tps, B, T, steps, nz, None, 0.7, out) != 0
        assert _raw(cfm, m, ptrs, tps, 0, T, steps, nz, None, 0.7, out) != 0
        assert _raw(cfm, m, ptrs, tps, B, T, steps, None, None, 0.7, out) != 0
        torch.cuda.synchronize()
        assert torch.isnan(out).all()
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            cfm.inference_rows(mu.to(DEV), ps, steps, noise=noise, inference_cfg_rate=bad)
        with pytest.raises(ValueError):
            cfm.inference_guided(mu.to(DEV), None, ps[2].expand(B, -1, -1), steps, inference_cfg_rate=bad)
    with pytest.raises(ValueError):
        cfm.inference_guided(mu[:, :4].to(DEV), None, ps[2].expand(B, -1, -1), steps, inference_cfg_rate=0.5)   # prompt longer than T
    got = cfm.inference_guided(mu.to(DEV), None, ps[2].expand(B, -1, -1), steps, inference_cfg_rate=0.5)
    assert got.shape == (B, md, T) and torch.isfinite(got).all()


def test_fp16_production_dit_guided_at_chunk_length():
    """DiT 1024 x 22, T = 934, fp16, 2 Euler steps, r = 0.7, the inputs of _parity.dit_v3_chunk_case() (Tp = 468): one request
    = 2 DiT rows = 1868 GEMM rows, whose routes differ from both the 934-row and the small cases, and 2 x 16 (row, head)
    pairs over the XCDs.  Against the helper in fp32 on 8 host threads: the fp16 DiT bar."""
    cfg, sd, mu, prompt, noise, steps, _ = dit_v3_chunk_case()
    torch.set_num_threads(8)
    ref = _cfg_ref.cfm_inference_cfg(sd, cfg, mu, prompt, steps, noise.clone(), 0.7)
    out = _cfm(cfg, sd, torch.float16).inference_rows(mu.to(DEV), [prompt.to(DEV)], steps, noise=noise,
                                                      inference_cfg_rate=0.7).float().cpu()
    _check_fp16_row(out, ref, 468, "fp16 depth-22 DiT guided r = 0.7 (Tp = 468)")
