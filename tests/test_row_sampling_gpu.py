"""GPU: per-row sampling parameters in the AR decode (gsv_t2s_set_row_sampling, gsv_op_sample_rows, run_batch(mixed_sampling)).

* the sampler alone, every branch of sample_core side by side in one launch, integer-exact against the oracle per row;
* fp32 launch path: a row of a mixed launch decodes what it decodes in a uniform launch with its setting;
* fp16 persistent engine: every executed step of every row replayed by the oracle on the dumped logits, and the same
  mixed-against-uniform equality;
* B copies of the scalars are bit-identical to not setting rows, and the rows apply to one decode only;
* bad values and a wrong row count are refused before anything is launched;
* run_batch(mixed_sampling=True) returns what run_batch returns, in one AR launch instead of four.

Top-p at a boundary is unpinned within ~1e-6 of top_p, so every comparison against the oracle first
checks, on the host, that the oracle's cumulative mass stays 1e-4 away from top_p at the cut: a violation is a bad input
(pick another seed), not a parity failure.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from test_t2s_ragged_gpu import _dev, _engine, _rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# the nine tuples of test_t2s_gpu.test_sampling_kernel_matches_oracle: (top_k, top_p, temperature, repetition_penalty)
NINE = [(1, 1.0, 1.0, 1.35), (5, 1.0, 1.0, 1.35), (15, 0.9, 0.8, 1.35), (0, 0.7, 1.3, 1.0), (0, 1.0, 1.0, 1.2),
        (20, 0.99, 1e-6, 1.35), (15, 1.0, 0.8, 1.35), (100, 1.0, 1.0, 1.2), (2, 1.0, 1.0, 1.0)]
# the decode tests cycle through four settings: greedy, top-k, top-p with penalty 1.0 (no penalty for that row), top-p alone
FOUR = [(1, 1.0, 1.0, 1.35), (15, 1.0, 1.0, 1.35), (5, 0.8, 0.9, 1.0), (0, 0.6, 1.2, 1.2)]
MARGIN = 1e-4
SAMPLER_SEED = {(1025, 18, 40): 0, (65, 9, 12): 0}     # chosen on the CPU so that the top-p margin guard holds


def _top_p_margin(logits_row, prev_row, rp, top_p):
    """distance of the oracle's cumulative mass (sorted, after the repetition penalty, before the temperature) from top_p"""
    from oracle.t2s_oracle import apply_repetition_penalty
    x = apply_repetition_penalty(logits_row[None], prev_row[None], rp)
    cum = torch.cumsum(torch.softmax(torch.sort(x, descending=True)[0], dim=-1), dim=-1)
    return float((cum - top_p).abs().min())


def _oracle_row(logits_row, prev_row, noise_row, setting):
    """(sampled token, argmax of the penalised logits) of one row under its own setting"""
    from oracle.t2s_oracle import apply_repetition_penalty, sample
    k, p, t, rp = setting
    s, _ = sample(logits_row[None].clone(), prev_row[None], noise=noise_row[None], top_k=k if k > 0 else None, top_p=p,
                  temperature=t, repetition_penalty=rp)
    a = torch.argmax(apply_repetition_penalty(logits_row[None], prev_row[None], rp), dim=-1)
    return int(s[0, 0]), int(a[0])


def _sampler_inputs(V, B, prev_len, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, V, generator=g) * 3
    for b in range(B):
        if NINE[b % 9][1] < 1.0:
            # tie-free, and twice as wide: at 1024 tokens and scale 3 the token that crosses top_p = 0.99 has a probability
            # below 1e-4, so no draw can keep both of its neighbours in the cumulative sum 1e-4 away from top_p
            logits[b] *= 2
        else:                           # ties, a masked token and both zeros, as the scalar test builds them
            logits[b] = logits[b].round(decimals=1)
            logits[b, 3], logits[b, 5], logits[b, 7] = -float("inf"), -0.0, 0.0
    prev = torch.randint(0, V - 1, (B, prev_len), generator=g)
    noise = torch.empty(B, V).exponential_(1, generator=g).clamp_min(1e-10)
    return logits, prev, noise


@pytest.mark.parametrize("V,B,prev_len", [(1025, 18, 40), (65, 9, 12)])
def test_sampler_rows_match_the_oracle_row_by_row(V, B, prev_len):
    from gsv import _lib
    _lib.init(0)
    logits, prev, noise = _sampler_inputs(V, B, prev_len, SAMPLER_SEED[(V, B, prev_len)])
    Veff = V - 1
    settings = [NINE[b % 9] for b in range(B)]
    for b, (k, p, t, rp) in enumerate(settings):
        if p < 1.0:
            m = _top_p_margin(logits[b, :Veff], prev[b], rp, p)
            assert m >= MARGIN, f"bad input: row {b} (top_p {p}) has cumulative mass within {m:.2e} of top_p; pick another seed"
    ref = [_oracle_row(logits[b, :Veff], prev[b], noise[b], settings[b]) for b in range(B)]
    rows = (_lib.RowSampling * B)(*[_lib.RowSampling(*s) for s in settings])
    lg_d, pv_d, nz_d = logits.to(DEV).contiguous(), prev.to(DEV, torch.int32).contiguous(), noise.to(DEV).contiguous()
    out_s = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    out_a = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().gsv_op_sample_rows(lg_d.data_ptr(), B, V, Veff, pv_d.data_ptr(), prev_len, rows, 0, nz_d.data_ptr(),
                                             0, out_s.data_ptr(), out_a.data_ptr(), None), "gsv_op_sample_rows")
    torch.cuda.synchronize()
    got = list(zip(out_s.cpu().tolist(), out_a.cpu().tolist()))
    for b in range(B):
        assert got[b] == ref[b], f"row {b} with {settings[b]}: (sample, argmax) {got[b]}, oracle {ref[b]}"


@pytest.fixture(scope="module")
def small():
    from oracle import cases
    cfg, sd, *_ = cases.t2s_case_inputs(cases.T2S_CASES["t2s_small_greedy"])
    return cfg, sd, _engine(cfg, sd, torch.float32, max_batch=64, max_seq=320)


@pytest.fixture(scope="module")
def v2():
    from gsv import synthetic as S
    cfg = S.T2S_V2_CONFIG
    sd = S.make_t2s_state_dict(cfg, seed=0, suppress_eos=True)
    return cfg, sd, _engine(cfg, sd, torch.float16, max_batch=128, max_seq=320)


IGNORED = dict(top_k=3, top_p=0.5, temperature=2.0, repetition_penalty=2.0)     # the scalars a mixed launch must not read


def _kw(setting):
    return dict(top_k=setting[0], top_p=setting[1], temperature=setting[2], repetition_penalty=setting[3])


def _assert_mixed_equals_uniform(eng, xd, pd, bd, ym, im, settings, **common):
    """every row of the mixed launch (ym, im) against the uniform launch with its setting and the same keys / noise"""
    for s in sorted(set(settings)):
        yu, iu = eng.infer_panel_batch_infer(xd, None, pd, bd, **_kw(s), **common)
        for b, sb in enumerate(settings):
            if sb == s:
                assert iu[b] == im[b] and yu[b].tolist() == ym[b].tolist(), f"row {b} with {s} differs from the uniform launch"


@pytest.mark.parametrize("B", [5, 33])
def test_fp32_mixed_launch_equals_uniform_launches(small, B):
    cfg, sd, eng = small
    xs, berts, prompts = _rows(cfg, B, seed=31 + B, zh_bert=True)
    xd, bd = _dev(xs, berts)
    pd = [p.to(DEV) for p in prompts]
    settings = [FOUR[b % 4] for b in range(B)]
    common = dict(early_stop_num=24, rng_keys=[(1000 + 7 * b, (3 * b + 1) % 6) for b in range(B)])
    ym, im = eng.infer_panel_batch_infer(xd, None, pd, bd, row_sampling=settings, **IGNORED, **common)
    assert eng.decode_info()[0] == 0
    _assert_mixed_equals_uniform(eng, xd, pd, bd, ym, im, settings, **common)
    assert len({tuple(y.tolist()[p.numel():]) for y, p in zip(ym, prompts)}) > 1


@pytest.mark.parametrize("B", [32, 96])
def test_fp16_engine_every_step_matches_the_oracle(v2, B):
    cfg, sd, eng = v2
    steps, V = 16, cfg["model"]["vocab_size"]
    xs, berts, prompts = _rows(cfg, B, seed=B + 3, zh_bert=True)
    xd, bd = _dev(xs, berts)
    pd = [p.to(DEV) for p in prompts]
    settings = [FOUR[b % 4] for b in range(B)]
    g = torch.Generator().manual_seed(7 + B)
    noise = torch.empty(steps + 1, B, V).exponential_(1, generator=g).clamp_min(1e-10)
    common = dict(early_stop_num=steps, noise=noise)
    ym, im = eng.infer_panel_batch_infer(xd, None, pd, bd, row_sampling=settings, dump_logits=True, **IGNORED, **common)
    mode = eng.decode_info()[0]
    _, fallbacks, _ = eng.engine_stats()
    assert mode == 1, "the persistent engine must run the mixed batch"
    assert fallbacks == 0
    L = eng.last_logits_dump.cpu()
    drawn = eng.last_drawn_dump.cpu()
    assert L.shape == (steps + 1, B, V) and torch.isfinite(L).all()
    executed, worst = 0, 1.0
    for b in range(B):
        P, hist = prompts[b].numel(), ym[b].cpu()
        for s in range(steps + 1):
            if drawn[s, b, 0] < 0:
                continue
            assert s <= im[b], f"row {b} ran step {s} after finishing at {im[b]}"
            Veff = V - 1 if s < 1 else V
            prev = hist[:P + s]
            k, p, t, rp = settings[b]
            if p < 1.0:
                m = _top_p_margin(L[s, b, :Veff], prev, rp, p)
                worst = min(worst, m)
                assert m >= MARGIN, f"bad input: step {s} row {b} (top_p {p}) has cumulative mass within {m:.2e} of top_p"
            ref = _oracle_row(L[s, b, :Veff], prev, noise[s, b], settings[b])
            assert (int(drawn[s, b, 0]), int(drawn[s, b, 1])) == ref, f"step {s} row {b} with {settings[b]}"
            executed += 1
    print(f"[row sampling] B = {B}: {executed} (step, row) samples replayed; smallest top-p margin {worst:.2e}")
    assert executed == B * (steps + 1) and im == [steps] * B
    _assert_mixed_equals_uniform(eng, xd, pd, bd, ym, im, settings, **common)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_rows_equal_to_the_scalars_are_bit_identical_and_last_one_decode(v2, small, dtype):
    cfg, sd, eng = v2 if dtype == torch.float16 else small
    B, steps = 32, 20
    xs, berts, prompts = _rows(cfg, B, seed=5, zh_bert=True)
    xd, bd = _dev(xs, berts)
    pd = [p.to(DEV) for p in prompts]
    s0 = (15, 0.9, 0.8, 1.35)
    common = dict(early_stop_num=steps, seed=1234, dump_logits=True)
    ya, ia = eng.infer_panel_batch_infer(xd, None, pd, bd, **_kw(s0), **common)
    la = eng.last_logits_dump.cpu().numpy()
    yb, ib = eng.infer_panel_batch_infer(xd, None, pd, bd, row_sampling=[s0] * B, **_kw(s0), **common)
    lb = eng.last_logits_dump.cpu().numpy()
    assert eng.decode_info()[0] == (1 if dtype == torch.float16 else 0)
    assert ia == ib and [y.tolist() for y in ya] == [y.tolist() for y in yb]
    assert np.array_equal(la, lb)
    # other rows change the draws, and the decode after it is back on the scalars
    yc, _ = eng.infer_panel_batch_infer(xd, None, pd, bd, row_sampling=[FOUR[0]] * B, **_kw(s0), **common)
    assert [y.tolist() for y in yc] != [y.tolist() for y in ya]
    yd, idd = eng.infer_panel_batch_infer(xd, None, pd, bd, **_kw(s0), **common)
    assert idd == ia and [y.tolist() for y in yd] == [y.tolist() for y in ya]
    assert np.array_equal(eng.last_logits_dump.cpu().numpy(), la)


def test_bad_rows_and_a_wrong_row_count_are_refused_before_any_launch(small):
    from gsv import _lib
    cfg, sd, eng = small
    B = 5
    xs, berts, prompts = _rows(cfg, B, seed=9, zh_bert=False)
    xd, bd = _dev(xs, berts)
    pd = [p.to(DEV) for p in prompts]
    kw = dict(early_stop_num=8, **_kw(FOUR[1]))
    good, _ = eng.infer_panel_batch_infer(xd, None, pd, bd, seed=3, **kw)
    l = _lib.lib()
    nan, inf = float("nan"), float("inf")
    bad = [(-1, 1.0, 1.0, 1.35), (5, 0.0, 1.0, 1.35), (5, 1.5, 1.0, 1.35), (5, nan, 1.0, 1.35), (5, 1.0, -0.5, 1.35),
           (5, 1.0, inf, 1.35), (5, 1.0, nan, 1.35), (5, 1.0, 1.0, 0.0), (5, 1.0, 1.0, -1.0), (5, 1.0, 1.0, inf),
           (5, 1.0, 1.0, nan)]
    out_tokens = torch.zeros(B, 9, dtype=torch.int32, device=DEV)
    out_len = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    for t in bad:
        rows = (_lib.RowSampling * B)(*([_lib.RowSampling(*FOUR[1])] * (B - 1) + [_lib.RowSampling(*t)]))
        assert l.gsv_t2s_set_row_sampling(eng._h, rows, B) != 0, f"{t} was accepted"
        assert b"row 4" in l.gsv_last_error()
        with pytest.raises(RuntimeError, match="gsv_t2s_set_row_sampling"):
            eng.infer_panel_batch_infer(xd, None, pd, bd, row_sampling=[FOUR[1]] * (B - 1) + [t], seed=3, **kw)
    ok = (_lib.RowSampling * B)(*[_lib.RowSampling(*FOUR[1])] * B)
    assert l.gsv_t2s_set_row_sampling(eng._h, ok, 0) != 0 and l.gsv_t2s_set_row_sampling(eng._h, ok, 65) != 0
    assert l.gsv_t2s_set_row_sampling(eng._h, None, B) != 0
    # a row count that is not the batch's: the decode is refused, nothing is written
    assert l.gsv_t2s_set_row_sampling(eng._h, ok, B - 1) == 0
    sp = _lib.SamplingParams(15, 1.0, 1.0, 1.35, 8, 1, 9, 3)
    steps = C.c_int(0)
    rc = l.gsv_t2s_decode(eng._h, C.byref(sp), None, 0, out_tokens.data_ptr(), out_len.data_ptr(), C.byref(steps),
                          C.c_void_p(eng.stream.cuda_stream))
    assert rc != 0 and b"gsv_t2s_set_row_sampling gave 4 rows for a batch of 5" in l.gsv_last_error()
    torch.cuda.synchronize()
    assert out_len.cpu().tolist() == [-1] * B and int(out_tokens.abs().sum()) == 0
    # the refused rows are gone: the engine decodes on the scalars as before
    again, _ = eng.infer_panel_batch_infer(xd, None, pd, bd, seed=3, **kw)
    assert [y.tolist() for y in again] == [y.tolist() for y in good]
    with pytest.raises(ValueError):
        eng.infer_panel_batch_infer(xd, None, pd, bd, row_sampling=[FOUR[1]] * (B + 1), seed=3, **kw)


def test_run_batch_mixed_sampling_is_one_launch_with_the_same_audio():
    """fp32, synthetic v2 weights, four voices and four settings.  Compared exactly (int16 arrays equal), the criterion of
    test_run_batch_gpu for run-against-run: the ids are bit-equal, so everything after them is too."""
    from test_run_batch_gpu import _build, _segs, _voice_args
    tts = _build("v2")
    base = dict(fragment_interval=0.01)
    reqs = []
    for i, (P, n_ph, n) in enumerate([(8, 6, 9), (23, 4, 7), (5, 7, 11), (12, 5, 6)]):
        voice = tts.make_voice(**_voice_args(i, P, n_ph, "v2"))
        reqs.append(dict(base, segments=_segs(30 + i, [n]), seed=3 + i, voice=voice, **_kw(FOUR[i])))
    calls = []
    run = tts.t2s_model._run

    def counted(*a, **kw):
        calls.append(kw.get("row_sampling"))
        return run(*a, **kw)

    tts.t2s_model._run = counted
    plain = tts.run_batch([dict(r) for r in reqs])
    assert len(calls) == 4 and all(c is None for c in calls)
    calls.clear()
    mixed = tts.run_batch([dict(r) for r in reqs], mixed_sampling=True)
    assert len(calls) == 1 and sorted(calls[0]) == sorted(FOUR)
    for r, ((sr_a, a), (sr_b, b)) in enumerate(zip(plain, mixed)):
        assert sr_a == sr_b and a.dtype == b.dtype == np.int16 and a.shape == b.shape
        assert np.array_equal(a, b), f"request {r}: mixed_sampling changed the audio"
        assert np.abs(a).max() > 0
    assert len({a.tobytes() for _, a in plain}) == 4
