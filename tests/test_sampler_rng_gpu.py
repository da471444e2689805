"""GPU: the sampler's own counter RNG (csrc/t2s_sample.h, the path production runs: no injected noise) against the host
mirror tests/_rng_ref.py.

* gsv_op_sample with noise = NULL: (sampled, argmax) of 4096 rows per launch equal the fp64 oracle fed the mirror's noise,
  at V = 65 (2 values per lane), 1025 (17) and 2048 (32), steps 0 / 1 / 1499, seeds with and without bits 31, 32 and 63, and
  three settings;
* keys found with the mirror at which u24 == 0 (the clamp: q = 1e-20) and u24 == 2**24 - 1 (the largest finite q);
* the token frequencies of 16384 kernel draws from one distribution, chi-square against the fp64 softmax: no guard, nothing
  skipped;
* both decode engines drawing for themselves (fp32 launch path, fp16 persistent engine) with per-row keys: every executed
  (step, row) replayed by the oracle on the dumped logits with the mirror's noise for (seed_b, row_b, step);
* RNG rows outside [0, 2**24) are refused before anything is launched.

Guards of the exact comparisons.  The device computes p and q in fp32, so a case is compared only where the fp64 reference's best
and second-best score p / q differ by at least 1e-4 relative (about 20x the fp32 rounding of expf at the exponents that
occur plus that of log1pf), and, for a top-p setting, where the cumulative mass stays 1e-4 away from top_p (the guard of
test_row_sampling_gpu).  At most 1 % of the cases of a launch may be left out; the share is asserted and printed.  The inputs
of the op tests are chosen on the CPU so that the reference alone stays inside that 1 %: the logits of the top-p launches are
scaled by 8 instead of 3 (the top-p rows of test_row_sampling_gpu: by 6), so that the tokens around the cut are far larger than
1e-4 (at scale 6 and 2047 tokens the guard left out 1.05 % of the rows, at scale 8 it leaves out 0.27 %).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _rng_ref as R
from test_row_sampling_gpu import FOUR, MARGIN, IGNORED, _kw
from test_t2s_ragged_gpu import _dev, _engine, _rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP = 1e-4                 # relative gap of the two best scores below which a case is not compared
CAP = 0.01                 # share of a launch that the guards may leave out
THREE = [(0, 1.0, 1.0, 1.0), (15, 1.0, 0.8, 1.35), (0, 0.9, 1.0, 1.0)]
STEPS = (0, 1, 1499)
SEEDS = (11, 0x80000000, 0x8000000180000003)
B_OP, PREV_LEN = 4096, 12


def _f32(x):
    """the value the device gets for a float parameter"""
    return float(np.float32(x))


def _margins(x, prev, rp, top_p):
    """test_row_sampling_gpu._top_p_margin for all rows of x at once"""
    from oracle.t2s_oracle import apply_repetition_penalty
    y = apply_repetition_penalty(x, prev, rp)
    cum = torch.cumsum(torch.softmax(torch.sort(y, descending=True)[0], dim=-1), dim=-1)
    return (cum - top_p).abs().min(dim=-1)[0]


def _oracle(x, prev, q, setting):
    """fp64 oracle on the rows of x [n][Veff] with noise q [n][>= Veff]: (sampled [n], argmax [n], comparable [n])"""
    from oracle.t2s_oracle import apply_repetition_penalty, sample
    k, p, t, rp = setting[0], _f32(setting[1]), _f32(setting[2]), _f32(setting[3])
    x = x.double()
    q = torch.as_tensor(q, dtype=torch.float64)[:, :x.shape[1]]
    s, probs = sample(x.clone(), prev, noise=q, top_k=k if k > 0 else None, top_p=p, temperature=t, repetition_penalty=rp)
    a = torch.argmax(apply_repetition_penalty(x, prev, rp), dim=-1)
    top2 = torch.topk(probs / q, 2, dim=-1)[0]
    ok = (top2[:, 0] - top2[:, 1]) >= GAP * top2[:, 0]
    if p < 1.0:
        ok &= _margins(x, prev, rp, p) >= MARGIN
    return s[:, 0].long(), a.long(), ok


def _op_inputs(V, setting):
    g = torch.Generator().manual_seed(1000 + V)
    logits = torch.randn(B_OP, V, generator=g) * (8 if setting[1] < 1.0 else 3)
    prev = torch.randint(0, V - 1, (B_OP, PREV_LEN), generator=g)
    return logits, prev


def _op_sample(logits, prev, V, Veff, setting, seed, step):
    from gsv import _lib
    _lib.init(0)
    n = logits.shape[0]
    sp = _lib.SamplingParams(setting[0], setting[1], setting[2], setting[3], -1, 1, 1500, seed)
    lg_d, pv_d = logits.to(DEV).contiguous(), prev.to(DEV, torch.int32).contiguous()
    out_s = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    out_a = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().gsv_op_sample(lg_d.data_ptr(), n, V, Veff, pv_d.data_ptr(), prev.shape[1], C.byref(sp), None, step,
                                        out_s.data_ptr(), out_a.data_ptr(), None), "gsv_op_sample")
    torch.cuda.synchronize()
    return out_s.cpu().long(), out_a.cpu().long()


def _launches(seed):
    """(step, setting) of a seed's three launches.  Over the three seeds every step meets every seed, and every setting meets
    every step and every seed"""
    j = SEEDS.index(seed)
    return [(st, THREE[(i + j) % 3]) for i, st in enumerate(STEPS)]


@pytest.mark.parametrize("seed", SEEDS, ids=hex)
@pytest.mark.parametrize("V", [65, 1025, 2048])
def test_op_draws_equal_the_mirror(V, seed):
    Veff = V - 1
    rows = np.arange(B_OP)
    worst = 0.0
    for step, setting in _launches(seed):
        logits, prev = _op_inputs(V, setting)
        q = R.noise(seed, rows, step, V)
        ref_s, ref_a, ok = _oracle(logits[:, :Veff], prev, q, setting)
        share = 1.0 - float(ok.double().mean())
        worst = max(worst, share)
        assert share <= CAP, f"bad input: V {V} step {step} seed {seed:#x} {setting}: the guards leave out {share:.2%} of the rows"
        got_s, got_a = _op_sample(logits, prev, V, Veff, setting, seed, step)
        bad = torch.nonzero(ok & ((got_s != ref_s) | (got_a != ref_a))).reshape(-1).tolist()
        assert not bad, (f"V {V} step {step} seed {seed:#x} {setting}: {len(bad)} rows differ, first row {bad[0]}: "
                         f"(sample, argmax) ({int(got_s[bad[0]])}, {int(got_a[bad[0]])}), "
                         f"oracle ({int(ref_s[bad[0]])}, {int(ref_a[bad[0]])})")
        assert len(set(got_s.tolist())) > 1              # the launch did draw: not one token for every row
    print(f"[sampler rng] V {V} seed {seed:#x}: 3 launches of {B_OP} rows compared; largest share left out by the guards "
          f"{worst:.3%}")


# Keys of seed 1234 at the two ends of u, found with the mirror: for every row 0 .. 63, R.uniform24(1234, row, steps 0 .. 1499,
# 1024) and np.nonzero(u == 0) / np.nonzero(u == 2**24 - 1) (9.8e7 draws, each end expected about six times; ~3 s).
EXT_SEED = 1234
U_ZERO = (21, 212, 498)         # (row, step, v) with u24 == 0: q is the clamp 1e-20
U_MAX = (2, 1056, 856)          # (row, step, v) with u24 == 2**24 - 1: q = 24 ln 2, the largest finite value


def test_extreme_keys_are_what_the_mirror_says():
    """host only (kept with the GPU tests it serves): the committed keys have the u they are named for"""
    r, s, v = U_ZERO
    assert R.uniform24_int(EXT_SEED, r, s, v) == 0 and R.noise(EXT_SEED, r, s, 1024)[v] == 1e-20
    r, s, v = U_MAX
    assert R.uniform24_int(EXT_SEED, r, s, v) == R.U24_MAX
    assert R.uniform24_int(EXT_SEED, r, s, v + 1) < R.U24_MAX


def test_u_zero_wins_through_the_clamp():
    row, step, v = U_ZERO
    V, Veff, n = 1025, 1024, 32
    assert row < n
    # no filter: token v holds about 1e-6 of the mass and wins with p / 1e-20; every other row of the launch draws as the oracle
    # says, none of them v (its chance there is 1e-6)
    x = torch.zeros(n, V)
    x[:, v] = -7.0
    # top-k 15 at temperature 0.8: 14 tokens at 10, v as the 15th at 1.2 (1.2e-6 of the kept mass), the rest at -5
    y = torch.full((n, V), -5.0)
    y[:, 100:114] = 10.0
    y[:, v] = 1.2
    prev = torch.zeros(n, 4, dtype=torch.int64)          # token 0 only: the penalty touches none of the kept tokens
    for logits, setting in ((x, THREE[0]), (y, THREE[1])):
        q = R.noise(EXT_SEED, np.arange(n), step, V)
        ref_s, ref_a, ok = _oracle(logits[:, :Veff], prev, q, setting)
        p_v = float(torch.softmax(logits[row, :Veff].double() / _f32(setting[2]), -1)[v]) if setting[0] == 0 else \
            float(np.exp((1.2 - 10.0) / _f32(0.8)) / 14.0)
        assert 5e-7 < p_v < 2e-6 and int(ref_s[row]) == v and bool(ok[row])
        got_s, got_a = _op_sample(logits, prev, V, Veff, setting, EXT_SEED, step)
        assert int(got_s[row]) == v, f"{setting}: row {row} drew {int(got_s[row])}, the clamped token is {v}"
        assert torch.equal(got_s[ok], ref_s[ok]) and torch.equal(got_a[ok], ref_a[ok])
        assert int((got_s == v).sum()) == 1


def test_u_max_is_the_largest_finite_noise():
    row, step, v = U_MAX
    V, Veff, n = 1025, 1024, 8
    w = v + 1
    q = R.noise(EXT_SEED, np.arange(n), step, V)
    q_v, q_w = float(q[row, v]), float(q[row, w])
    assert abs(q_v - 24 * np.log(2.0)) < 1e-12 and q_w < q_v
    prev = torch.zeros(n, 4, dtype=torch.int64)
    # two tokens hold the mass.  Equal logits: v, with the largest q there is, loses to its neighbour
    x = torch.full((n, V), -60.0)
    x[:, v], x[:, w] = 0.0, 0.0
    got_s, _ = _op_sample(x, prev, V, Veff, THREE[0], EXT_SEED, step)
    assert int(got_s[row]) == w
    # ... but q stays finite: with the neighbour's logit lowered by log(q_v / q_w) + 0.5, v's score is e**0.5 times the larger
    x[:, w] = -(float(np.log(q_v / q_w)) + 0.5)
    ref_s, _, ok = _oracle(x[:, :Veff], prev, q, THREE[0])
    assert int(ref_s[row]) == v and bool(ok[row])
    got_s, _ = _op_sample(x, prev, V, Veff, THREE[0], EXT_SEED, step)
    assert int(got_s[row]) == v


def test_kernel_draws_follow_the_softmax():
    lg = R.race_logits()                                  # 64 tokens at scale 1.5
    V, Veff, n = 65, 64, 8192
    x = torch.zeros(n, V)
    x[:, :Veff] = torch.from_numpy(lg)
    prev = torch.zeros(n, 4, dtype=torch.int64)
    counts = np.zeros(Veff, dtype=np.int64)
    per_step = []
    for step in (2, 1499):
        got_s, _ = _op_sample(x, prev, V, Veff, THREE[0], SEEDS[2], step)
        assert int(got_s.min()) >= 0 and int(got_s.max()) < Veff
        per_step.append(got_s)
        counts += np.bincount(got_s.numpy(), minlength=Veff)
    assert not torch.equal(per_step[0], per_step[1])
    x2, df = R.chi2_counts(counts, R.softmax64(lg))
    print(f"[sampler rng] {counts.sum()} kernel draws over {Veff} tokens: chi-square = {x2:.1f} (bar {R.chi2_bar(df):.1f}, df {df})")
    assert x2 <= R.chi2_bar(df)


# ---- the engines drawing for themselves ------------------------------------------------------------------------------------
KEY_SEEDS = [0x80000000, 0x100000000, 0x8000000000000000, 0x8000000180000003, 0xFFFFFFFFFFFFFFFF, 11]
KEY_ROWS = [0, 63, 1027, 2051, 1024 * 15 + 127, (1 << 24) - 1]


def _keys(B):
    """seeds with bits 31, 32 and 63 set (and one without), rows on and off the best_of stride up to the last one"""
    return [(KEY_SEEDS[b % 6] + (b // 6), (KEY_ROWS[(b + b // 6) % 6] + 3 * (b // 6)) % (1 << 24)) for b in range(B)]


def _replay(eng, cfg, B, steps, seed, expect_mode):
    V = cfg["model"]["vocab_size"]
    xs, berts, prompts = _rows(cfg, B, seed=seed, zh_bert=True)
    xd, bd = _dev(xs, berts)
    pd = [p.to(DEV) for p in prompts]
    settings = [FOUR[b % 4] for b in range(B)]
    keys = _keys(B)
    ym, im = eng.infer_panel_batch_infer(xd, None, pd, bd, row_sampling=settings, dump_logits=True, early_stop_num=steps,
                                         rng_keys=keys, **IGNORED)
    assert eng.decode_info()[0] == expect_mode
    if expect_mode == 1:
        assert eng.engine_stats()[1] == 0, "the persistent engine fell back"
    L, drawn = eng.last_logits_dump.cpu(), eng.last_drawn_dump.cpu()
    assert L.shape == (steps + 1, B, V)
    executed = skipped = 0
    for b in range(B):
        P, hist = prompts[b].numel(), ym[b].cpu()
        ran = [s for s in range(steps + 1) if drawn[s, b, 0] >= 0]
        assert ran == list(range(im[b] + 1)), f"row {b} finished at {im[b]} and ran steps {ran}"
        q = R.noise(keys[b][0], keys[b][1], np.array(ran), V)                     # [steps run][V]
        for s in ran:
            Veff = V - 1 if s < 1 else V
            ref_s, ref_a, ok = _oracle(L[s, b, :Veff][None], hist[None, :P + s], q[s][None], settings[b])
            executed += 1
            if not bool(ok[0]):
                skipped += 1
                continue
            assert (int(drawn[s, b, 0]), int(drawn[s, b, 1])) == (int(ref_s[0]), int(ref_a[0])), \
                f"step {s} row {b} key ({keys[b][0]:#x}, {keys[b][1]}) with {settings[b]}"
    share = skipped / executed
    print(f"[sampler rng] engine mode {expect_mode}, B = {B}: {executed} (step, row) draws replayed, "
          f"{skipped} left out by the guards ({share:.2%})")
    assert share <= CAP
    assert len({tuple(y.tolist()[p.numel():]) for y, p in zip(ym, prompts)}) > 1
    return executed


def test_fp32_launch_path_draws_equal_the_mirror():
    from oracle import cases
    cfg, sd, *_ = cases.t2s_case_inputs(cases.T2S_CASES["t2s_small_greedy"])
    eng = _engine(cfg, sd, torch.float32, max_batch=8, max_seq=320)
    assert _replay(eng, cfg, B=5, steps=24, seed=36, expect_mode=0) > 5 * 12


def test_fp16_engine_draws_equal_the_mirror():
    from gsv import synthetic as S
    cfg = S.T2S_V2_CONFIG
    sd = S.make_t2s_state_dict(cfg, seed=0, suppress_eos=True)
    eng = _engine(cfg, sd, torch.float16, max_batch=32, max_seq=320)
    assert _replay(eng, cfg, B=32, steps=16, seed=35, expect_mode=1) == 32 * 17


def test_rng_rows_outside_24_bits_are_refused_before_any_launch():
    from gsv import _lib
    from oracle import cases
    cfg, sd, *_ = cases.t2s_case_inputs(cases.T2S_CASES["t2s_small_greedy"])
    eng = _engine(cfg, sd, torch.float32, max_batch=8, max_seq=320)
    B = 5
    xs, berts, prompts = _rows(cfg, B, seed=9, zh_bert=False)
    xd, bd = _dev(xs, berts)
    pd = [p.to(DEV) for p in prompts]
    kw = dict(early_stop_num=8, **_kw(FOUR[1]))
    edge = [(3, 0), (3, 1), (3, 1027), (3, (1 << 24) - 1), (3, 4)]
    good, gi = eng.infer_panel_batch_infer(xd, None, pd, bd, rng_keys=edge, **kw)
    l = _lib.lib()
    seeds_h = (C.c_uint64 * B)(*[3] * B)
    for bad in (-1, 1 << 24, (1 << 24) + 5, -(1 << 31), (1 << 31) - 1):
        rows_h = (C.c_int32 * B)(*([0] * (B - 1) + [bad]))
        assert l.gsv_t2s_set_row_rng(eng._h, C.cast(seeds_h, C.c_void_p), C.cast(rows_h, C.c_void_p), B) != 0, f"row {bad} accepted"
        err = l.gsv_last_error()
        assert b"row 4" in err and str(bad).encode() in err, err
        with pytest.raises(RuntimeError, match="gsv_t2s_set_row_rng"):
            eng.infer_panel_batch_infer(xd, None, pd, bd, rng_keys=[(3, 0)] * (B - 1) + [(3, bad)], **kw)
    # nothing was kept: a decode without keys draws with (seed, b), and the same keys give the same tokens as before
    plain, _ = eng.infer_panel_batch_infer(xd, None, pd, bd, seed=3, **kw)
    keyed, _ = eng.infer_panel_batch_infer(xd, None, pd, bd, rng_keys=[(3, b) for b in range(B)], **kw)
    assert [y.tolist() for y in plain] == [y.tolist() for y in keyed]
    again, ai = eng.infer_panel_batch_infer(xd, None, pd, bd, rng_keys=edge, **kw)
    assert ai == gi and [y.tolist() for y in again] == [y.tolist() for y in good]
    # a session refuses the row at the admission: the slot stays free and the session goes on
    with eng.open_session(4, early_stop_num=8, **_kw(FOUR[1])) as ses:
        row = lambda b, key: dict(x=xd[b], bert=bd[b], prompt=pd[b], key=key)
        for bad in (-1, 1 << 24):
            with pytest.raises(RuntimeError, match="gsv_t2s_session_admit"):
                ses.admit([row(0, (3, 0)), row(1, (3, bad))])
            err = l.gsv_last_error()
            assert b"row 1" in err and str(bad).encode() in err, err
            assert ses.live == 0 and int(ses.state()[1].sum()) == 0
        ses.admit([row(b, edge[b]) for b in range(4)])
        done = {}
        while ses.live:
            for t, y, n in ses.advance(4):
                done[t] = (y.tolist(), n)
        for b in range(4):
            assert done[b] == (good[b].tolist(), gi[b]), f"row {b} of the session differs from the static launch"
