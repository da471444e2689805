"""GPU: LoRA adapters held beside the DiT's base weights (gsv_cfm_adapter_*, gsv_cfm_inference_adapted, CFM.inference_rows(
adapters=...)): rows of one flow-matching pass that each run their own fine-tuned voice, against the oracle run on each row
alone with that voice's weights merged in fp32 (tests/_lora_ref.py: process_ckpt.merge_lora_v3).

The synthetic adapters (tests/_lora_ref.py, amplitude 2.5; the reasoning behind the amplitude is there) were chosen on the
CPU with the oracle alone: on the rows of this file a merged row differs from the base row by 2.2 - 3.7 max-abs and 36 - 63 %
relative rms (the fp16 bar is 0.15 / 3 %, the fp32 bar 2e-3), and its generated frames keep an rms of 1.3 - 1.6 (base: 1.4).
_refs() asserts that again."""
import ctypes as C
import functools

import pytest
import torch

import _cfg_ref
import _lora_ref as L
from _parity import rel_rms
from gsv import synthetic as S
from oracle import cfm_oracle
from test_cfm_rows_gpu import DEV, _cfm, _check_fp16_row, _rows, _small

pytestmark = pytest.mark.gpu
RANKS = ((4, 11), (16, 12))                 # (rank, seed) of adapters 0 and 1
SLOTS = [0, 1, -1, 1, 0]
RATE = 0.7


@functools.lru_cache(maxsize=None)
def _adapters():
    _, sd, _, _, _ = _small()
    return tuple(L.make_adapter(sd, r, seed) for r, seed in RANKS)


@functools.lru_cache(maxsize=None)
def _refs(rate=0.0):
    """per row: the oracle on that row alone with the weights its slot stands for; once per session and rate.  Also checks
    that the adapters move every adapted row by more than 10 x the bars."""
    cfg, sd, T, tps, steps = _small()
    mu, prompts, noise = _rows(cfg, T, tps, "rows")
    weights = {-1: sd}
    for s, (r, _) in enumerate(RANKS):
        weights[s] = L.merged(sd, _adapters()[s], r)

    def run(w, b):
        if rate:
            return _cfg_ref.cfm_inference_cfg(w, cfg, mu[b:b + 1], prompts[b], steps, noise[b:b + 1].clone(), rate)
        return cfm_oracle.cfm_inference(w, cfg, mu[b:b + 1], prompts[b], steps, noise[b:b + 1].clone())
    refs = tuple(run(weights[s], b) for b, s in enumerate(SLOTS))
    for b, s in enumerate(SLOTS):
        if s >= 0 and tps[b] < T:
            base = run(sd, b)
            gen = refs[b][..., tps[b]:]
            d, rel, rms = (refs[b] - base).abs().max().item(), rel_rms(gen, base[..., tps[b]:]), gen.pow(2).mean().sqrt().item()
            print(f"[lora] rate {rate} row {b} slot {s}: merged - base max-abs {d:.2f}, relative rms {rel * 100:.0f} %, rms {rms:.2f}")
            assert torch.isfinite(refs[b]).all() and 0.3 < rms < 3.0
            assert d >= 10 * 0.15 and rel >= 10 * 0.03
    return refs


def _engine(dtype):
    cfg, sd, _, _, _ = _small()
    cfm = _cfm(cfg, sd, dtype)
    slots = [cfm.add_adapter(a, r) for a, (r, _) in zip(_adapters(), RANKS)]
    assert slots == [0, 1] and cfm.estimator.adapter_count() == 2
    return cfm


def _run(cfm, slots, rate=0, **kw):
    cfg, _, T, tps, steps = _small()
    mu, prompts, noise = _rows(cfg, T, tps, "rows")
    return cfm.inference_rows(mu.to(DEV), [p.to(DEV) for p in prompts], steps, noise=noise, inference_cfg_rate=rate,
                              adapters=slots, **kw)


@pytest.mark.parametrize("rate", [0.0, RATE], ids=["unguided", "guided"])
def test_fp32_adapted_rows_match_their_merged_oracle(rate):
    """slots [0, 1, base, 1, 0]: every row within the fp32 CFM bar (2e-3 max-abs) of the oracle with its own merged weights
    (the base weights for the row without a slot); prompt frames exactly 0.  Guided: rate 0.7, the twin takes the row's slot."""
    _, _, T, tps, _ = _small()
    out = _run(_engine(torch.float32), [None if s < 0 else s for s in SLOTS], rate).cpu()
    for b, ref in enumerate(_refs(rate)):
        err = (out[b:b + 1] - ref).abs().max().item()
        print(f"[parity] fp32 rate {rate} row {b} (Tp = {tps[b]}, slot {SLOTS[b]}): max-abs error {err:.2e}")
        assert err <= 2e-3
        assert tps[b] == 0 or float(out[b, :, :tps[b]].abs().max()) == 0.0
    assert float(out[4].abs().max()) == 0.0


@pytest.mark.parametrize("rate", [0.0, RATE], ids=["unguided", "guided"])
def test_fp16_adapted_rows_match_their_merged_oracle(rate):
    """the same through the fp16 engine (MFMA delta kernel, fused attention): the fp16 DiT bar of test_cfm_rows_gpu.py"""
    _, _, _, tps, _ = _small()
    out = _run(_engine(torch.float16), SLOTS, rate).float().cpu()
    for b, ref in enumerate(_refs(rate)):
        _check_fp16_row(out[b:b + 1], ref, tps[b], f"fp16 rate {rate} row {b} (Tp = {tps[b]}, slot {SLOTS[b]})")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_base_paths_stay_bit_equal_and_rows_are_independent(dtype):
    """adapters=None and all -1 are the call without the keyword, bit for bit, on an engine that holds adapters; in a mixed
    pass the rows without a slot are bit-equal to the unadapted call; changing row 1's slot changes row 1 only; a repeated
    call is bit-identical.  The same guided."""
    _, _, _, tps, _ = _small()
    cfm = _engine(dtype)
    for rate in (0, RATE):
        plain = _run(cfm, None, rate)
        assert torch.equal(_run(cfm, [None] * 5, rate), plain) and torch.equal(_run(cfm, [-1] * 5, rate), plain)
        mixed = _run(cfm, SLOTS, rate)
        assert torch.equal(mixed, _run(cfm, SLOTS, rate)), "a repeated call"
        assert torch.equal(mixed[2], plain[2]) and torch.equal(mixed[4], plain[4])
        for b in (0, 1, 3):
            assert (mixed[b].float() - plain[b].float()).abs().max().item() > 0.5, f"row {b}: the adapter changed nothing"
        other = list(SLOTS)
        other[1] = 0
        moved = _run(cfm, other, rate)
        for b in (0, 2, 3, 4):
            assert torch.equal(moved[b], mixed[b]), f"row {b} changed with the slot of row 1"
        assert not torch.equal(moved[1], mixed[1])
    # the uniform entries take the keyword too
    cfg, _, T, _, steps = _small()
    mu, prompts, noise = _rows(cfg, T, tps, "rows")
    p = prompts[2].to(DEV)
    uni = cfm.inference(mu.to(DEV), None, p, steps, noise=noise, adapters=SLOTS)
    rows = cfm.inference_rows(mu.to(DEV), [p] * 5, steps, noise=noise, adapters=SLOTS)
    assert torch.equal(uni, rows)
    assert torch.equal(cfm.inference_guided(mu.to(DEV), None, p, steps, noise=noise, inference_cfg_rate=RATE, adapters=SLOTS),
                       cfm.inference_rows(mu.to(DEV), [p] * 5, steps, noise=noise, inference_cfg_rate=RATE, adapters=SLOTS))


def _raw(cfm, mu, ptrs, tps, slots, B, T, steps, noise, out, rate=0.0):
    from gsv import _lib
    dit = cfm.estimator
    rc = _lib.lib().gsv_cfm_inference_adapted(dit._h, mu.data_ptr(), (C.c_void_p * len(ptrs))(*ptrs), (C.c_int * len(tps))(*tps),
                                              (C.c_int * len(slots))(*slots) if slots is not None else None, B, T, steps,
                                              noise.data_ptr(), None, 1.0, rate, out.data_ptr(), C.c_void_p(dit.stream.cuda_stream))
    dit.stream.synchronize()
    return rc


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_store_lifecycle_and_refused_calls(dtype):
    """remove a slot and add another adapter into it; a removed slot, a slot out of range or beyond the cap and a non-finite
    rate return an error and write nothing (NaN-filled `out` stays NaN); NaN sentinels behind `out` survive a good call; a
    failed finalize leaves the store as it was; the cap holds."""
    from gsv import _lib
    cfg, sd, T, tps, steps = _small()
    B, md = len(tps), cfg["mel_dim"]
    mu, prompts, noise = _rows(cfg, T, tps, "rows")
    cfm = _engine(dtype)
    dit = cfm.estimator
    want = _run(cfm, SLOTS).float().reshape(-1)
    with torch.cuda.device(DEV):
        m, nz = mu.to(DEV).contiguous(), noise.to(DEV).contiguous()
        ps = [p.to(DEV).contiguous() for p in prompts]
        ptrs = [p.data_ptr() if p.shape[2] else None for p in ps]
        n, guard = B * md * T, 4096
        out = torch.full((n + guard,), float("nan"), device=DEV)
        torch.cuda.synchronize()
        assert _raw(cfm, m, ptrs, tps, SLOTS, B, T, steps, nz, out) == 0
        assert torch.equal(out[:n], want) and torch.isnan(out[n:]).all()
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        assert _raw(cfm, m, ptrs, tps, None, B, T, steps, nz, out) == 0            # NULL: every row the base model
        assert torch.equal(out[:n], _run(cfm, None).float().reshape(-1))
        # refused before anything is launched
        out.fill_(float("nan"))
        torch.cuda.synchronize()
        for bad in (2, _lib.CFM_MAX_ADAPTERS - 1, _lib.CFM_MAX_ADAPTERS, 10 ** 6, -2):
            sl = list(SLOTS)
            sl[3] = bad
            assert _raw(cfm, m, ptrs, tps, sl, B, T, steps, nz, out) != 0, bad
        assert _raw(cfm, m, ptrs, tps, SLOTS, B, T, steps, nz, out, rate=float("nan")) != 0
        cfm.remove_adapter(1)
        assert dit.adapter_count() == 1
        assert _raw(cfm, m, ptrs, tps, SLOTS, B, T, steps, nz, out) != 0, "a removed slot"
        torch.cuda.synchronize()
        assert torch.isnan(out).all()
    with pytest.raises(ValueError):
        _run(cfm, SLOTS)                                   # the host mirror: unknown slot
    with pytest.raises(ValueError):
        _run(cfm, SLOTS[:-1])                              # one entry per row
    with pytest.raises(ValueError):
        cfm.remove_adapter(1)
    # a failed finalize (a pair missing; a wrong rank; a name that is no adapted Linear) leaves the count where it was
    a16 = _adapters()[1]
    missing = {k: v for k, v in a16.items() if k != "transformer_blocks.1.attn.to_out.0.lora_B"}
    for bad, rank in ((missing, 16), (a16, 8), (dict(a16, **{"transformer_blocks.0.attn.nowhere.lora_A": a16[next(iter(a16))]}), 16)):
        with pytest.raises(RuntimeError):
            cfm.add_adapter(bad, rank)
        assert dit.adapter_count() == 1
    with pytest.raises(ValueError):
        cfm.add_adapter(a16, 0)
    with pytest.raises(ValueError):
        cfm.add_adapter(a16, _lib.LORA_MAX_RANK + 1)
    # the freed slot is reused: the rank-4 adapter again, now in slot 1 -> rows 1 and 3 equal what slot 0 gives them
    assert cfm.add_adapter(_adapters()[0], RANKS[0][0]) == 1 and dit.adapter_count() == 2
    assert torch.equal(_run(cfm, SLOTS), _run(cfm, [0, 0, -1, 0, 0]))
    # lora_alpha = rank / 2 halves the delta: the oracle merge with that lora_alpha
    cfm.remove_adapter(1)
    assert cfm.add_adapter(_adapters()[0], RANKS[0][0], alpha=RANKS[0][0] / 2) == 1
    got = _run(cfm, [None, 1, None, None, None]).float().cpu()
    ref = cfm_oracle.cfm_inference(L.merged(sd, _adapters()[0], RANKS[0][0], RANKS[0][0] / 2), cfg, mu[1:2], prompts[1], steps,
                                   noise[1:2].clone())
    assert (ref - _refs()[1]).abs().max().item() > 0.1, "lora_alpha changed nothing in the reference"
    if dtype == torch.float32:
        assert (got[1:2] - ref).abs().max().item() <= 2e-3
    else:
        _check_fp16_row(got[1:2], ref, tps[1], "fp16 lora_alpha = r / 2")
    # the cap: GSV_CFM_MAX_ADAPTERS live adapters, one more is refused and changes nothing
    for _ in range(_lib.CFM_MAX_ADAPTERS - 2):
        cfm.add_adapter(_adapters()[0], RANKS[0][0])
    assert dit.adapter_count() == _lib.CFM_MAX_ADAPTERS
    with pytest.raises(RuntimeError):
        cfm.add_adapter(_adapters()[0], RANKS[0][0])
    assert dit.adapter_count() == _lib.CFM_MAX_ADAPTERS
    sl = [_lib.CFM_MAX_ADAPTERS - 1, 1, -1, 1, 0]
    assert torch.equal(_run(cfm, sl)[0], _run(cfm, [0] * 5)[0]), "the last slot holds the rank-4 adapter too"


def test_fp16_real_width_mixed_ranks():
    """dim 1024, 16 heads, depth 2, T = 70 (two 64-frame tiles, the second masked), fp16: ranks 32 and 128 and a base row in
    one pass, each against its merged oracle at the fp16 DiT bar: the K = 1024 loop and the 3072 q|k|v columns at real width"""
    cfg = dict(S.small_dit_config(), dim=1024, heads=16, dim_head=64, depth=2)
    sd = S.make_dit_state_dict(cfg, seed=7)
    T, tps, steps = 70, [10, 0, 33], 2
    mu, prompts, noise = _rows(cfg, T, tps, "lora1024")
    ranks = ((32, 21), (128, 22))
    ads = [L.make_adapter(sd, r, seed) for r, seed in ranks]
    cfm = _cfm(cfg, sd, torch.float16)
    slots = [cfm.add_adapter(a, r) for a, (r, _) in zip(ads, ranks)]
    order = [slots[1], None, slots[0]]
    out = cfm.inference_rows(mu.to(DEV), [p.to(DEV) for p in prompts], steps, noise=noise, adapters=order).float().cpu()
    torch.set_num_threads(8)
    for b, s in enumerate(order):
        w = sd if s is None else L.merged(sd, ads[s], ranks[s][0])
        ref = cfm_oracle.cfm_inference(w, cfg, mu[b:b + 1], prompts[b], steps, noise[b:b + 1].clone())
        if s is not None:
            base = cfm_oracle.cfm_inference(sd, cfg, mu[b:b + 1], prompts[b], steps, noise[b:b + 1].clone())
            d, rel = (ref - base).abs().max().item(), rel_rms(ref[..., tps[b]:], base[..., tps[b]:])
            rms = ref[..., tps[b]:].pow(2).mean().sqrt().item()
            print(f"[lora] width 1024 row {b} rank {ranks[s][0]}: merged - base max-abs {d:.2f}, relative rms {rel * 100:.0f} %, rms {rms:.2f}")
            assert d >= 10 * 0.15 and rel >= 10 * 0.03 and 0.3 < rms < 3.0
        _check_fp16_row(out[b:b + 1], ref, tps[b], f"fp16 width 1024 row {b} (Tp = {tps[b]}, slot {s})")
