"""GPU: one AR decode over rows with different reference voices -- ragged prompt lengths P_b (gsv_t2s_prefill_ragged) and
per-row counter-RNG keys (gsv_t2s_set_row_rng).

* fp32 launch path: every row of a ragged batch (P_b in {1, 37, 100, 163}) decodes the ids the oracle gives for that row
  alone, at B = 5 and B = 33, with and without non-zero BERT features;
* fp16 persistent engine, teacher-forced on the fp32 ids: every step's logits within the band of
  test_t2s_engine_parity_gpu.py, at B = 32 (one quad) and B = 128 (four quads), mode 1 and no fallback;
* all P_b equal: the ragged entry is bit-identical (ids and logits) to gsv_t2s_prefill, fp16 and fp32;
* a row keyed (s, j) draws what row j of a uniform batch with seed s draws; no keys = keys (seed, b).
"""
import numpy as np
import pytest
import torch

from oracle import cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PLENS = (1, 37, 100, 163)


def _engine(cfg, sd, dtype, max_batch, max_seq):
    from gsv.AR.models.t2s_model import Text2SemanticDecoder
    m = Text2SemanticDecoder(cfg, device=DEV, dtype=dtype, max_batch=max_batch, max_seq=max_seq)
    m.load_state_dict(sd)
    return m


def _rows(cfg, B, seed, zh_bert, plens=PLENS, xlo=6, xhi=40):
    """B rows with distinct texts and prompts of lengths cycling through plens"""
    from gsv import synthetic as S
    m = cfg["model"]
    xl = S.hash_ints("rg_xlen", B, xhi - xlo, seed) + xlo
    xs = [torch.from_numpy(S.hash_ints(f"rg_x{i}", int(n), m["phoneme_vocab_size"], seed)).long() for i, n in enumerate(xl)]
    if zh_bert:
        berts = [S.hash_symmetric(f"rg_bert{i}", (1024, int(n)), 0.5, seed) for i, n in enumerate(xl)]
    else:
        berts = [torch.zeros(1024, int(n)) for n in xl]
    prompts = [torch.from_numpy(S.hash_ints(f"rg_p{i}", plens[i % len(plens)], m["vocab_size"] - 1, seed)).long()
               for i in range(B)]
    return xs, berts, prompts


def _dev(xs, berts):
    return [x.to(DEV) for x in xs], [b.to(DEV) for b in berts]


@pytest.fixture(scope="module")
def small():
    cfg, sd, *_ = cases.t2s_case_inputs(cases.T2S_CASES["t2s_small_greedy"])
    return cfg, sd, _engine(cfg, sd, torch.float32, max_batch=64, max_seq=320)


@pytest.mark.parametrize("B", [5, 33])
@pytest.mark.parametrize("zh_bert", [False, True])
def test_fp32_ragged_rows_bit_exact_vs_oracle_alone(small, B, zh_bert):
    from oracle.t2s_oracle import T2SOracle
    cfg, sd, eng = small
    xs, berts, prompts = _rows(cfg, B, seed=11 + B, zh_bert=zh_bert)
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, early_stop_num=40, repetition_penalty=1.35)
    xd, bd = _dev(xs, berts)
    ys, idxs = eng.infer_panel_batch_infer(xd, None, [p.to(DEV) for p in prompts], bd, **kw)
    orc = T2SOracle(sd, cfg)
    for b in range(B):
        oy, oi = orc.infer_panel_batch_infer([xs[b]], None, prompts[b].unsqueeze(0), [berts[b]], **kw)
        assert idxs[b] == oi[0], f"row {b} (P_b = {prompts[b].numel()}): {idxs[b]} tokens, oracle {oi[0]}"
        assert ys[b].cpu().tolist() == oy[0].tolist(), f"row {b} (P_b = {prompts[b].numel()}) differs from the oracle"


@pytest.fixture(scope="module")
def v2():
    from gsv import synthetic as S
    cfg = S.T2S_V2_CONFIG
    sd = S.make_t2s_state_dict(cfg, seed=0, suppress_eos=True)
    return cfg, sd


@pytest.mark.parametrize("B,steps", [(32, 60), (128, 24)])
def test_fp16_engine_ragged_teacher_forced_vs_fp32(v2, B, steps):
    cfg, sd = v2
    xs, berts, prompts = _rows(cfg, B, seed=B, zh_bert=True)
    xd, bd = _dev(xs, berts)
    pd = [p.to(DEV) for p in prompts]
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, early_stop_num=steps, repetition_penalty=1.35)
    e32 = _engine(cfg, sd, torch.float32, max_batch=64, max_seq=320)
    L32, tok = [], []
    for lo in range(0, B, 64):          # fp32 handles hold 64 rows: the reference logits come chunk by chunk
        hi = min(lo + 64, B)
        y, i = e32.infer_panel_batch_infer(xd[lo:hi], None, pd[lo:hi], bd[lo:hi], dump_logits=True, **kw)
        assert i == [steps] * (hi - lo)
        L32.append(e32.last_logits_dump.cpu().numpy())
        tok += [y_[pd[lo + k].numel():].to(torch.int32).cpu() for k, y_ in enumerate(y)]
    del e32
    torch.cuda.empty_cache()
    L32 = np.concatenate(L32, axis=1)
    tok = torch.stack(tok)
    e16 = _engine(cfg, sd, torch.float16, max_batch=128, max_seq=320)
    force = torch.zeros(B, steps + 1, dtype=torch.int32)
    force[:, :steps] = tok
    ys, idx = e16.infer_panel_batch_infer(xd, None, pd, bd, force_tokens=force, dump_logits=True, **kw)
    mode = e16.decode_info()[0]
    avail, fallbacks, _ = e16.engine_stats()
    assert mode == 1, "the persistent engine must run the ragged batch"
    assert fallbacks == 0
    assert idx == [steps] * B
    assert [y.cpu().tolist() for y in ys] == [torch.cat([p, t.long()]).tolist() for p, t in zip(prompts, tok)]
    L16 = e16.last_logits_dump.cpu().numpy()
    assert L16.shape == L32.shape == (steps + 1, B, cfg["model"]["vocab_size"])
    assert np.isfinite(L16).all()
    err = np.abs(L16 - L32).reshape(steps + 1, -1).max(1)
    print(f"[ragged] B = {B}: teacher-forced fp16 engine vs fp32 max {err.max():.3e} (step {err.argmax()}), "
          f"|logits| max {np.abs(L32).max():.1f}")
    assert err.max() <= 5e-2, f"engine logits leave the 5e-2 band at step {err.argmax()}"


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_uniform_prompts_through_the_ragged_entry_are_bit_identical(v2, dtype):
    cfg, sd = v2
    B, steps = 32, 30
    xs, berts, prompts = _rows(cfg, B, seed=5, zh_bert=True, plens=(57,))
    xd, bd = _dev(xs, berts)
    eng = _engine(cfg, sd, dtype, max_batch=32, max_seq=256)
    kw = dict(top_k=15, top_p=1.0, temperature=1.0, early_stop_num=steps, repetition_penalty=1.35, seed=1234)
    ya, ia = eng.infer_panel_batch_infer(xd, None, torch.stack(prompts).to(DEV), bd, dump_logits=True, **kw)
    la = eng.last_logits_dump.cpu().numpy()
    mode_a = eng.decode_info()[0]
    yb, ib = eng.infer_panel_batch_infer(xd, None, [p.to(DEV) for p in prompts], bd, dump_logits=True, **kw)
    lb = eng.last_logits_dump.cpu().numpy()
    mode_b = eng.decode_info()[0]
    assert mode_a == mode_b == (1 if dtype == torch.float16 else 0)
    assert ia == ib and [y.tolist() for y in ya] == [y.tolist() for y in yb]
    assert np.array_equal(la, lb), "logits of the ragged entry differ from the uniform one"


def test_row_rng_keys_follow_the_row_not_the_batch(small):
    cfg, sd, eng = small
    B = 9
    xs, berts, prompts = _rows(cfg, B, seed=23, zh_bert=True)
    xd, bd = _dev(xs, berts)
    pd = [p.to(DEV) for p in prompts]
    kw = dict(top_k=15, top_p=1.0, temperature=1.0, early_stop_num=30, repetition_penalty=1.35)
    keys = [(1000 + 7 * b, (3 * b + 1) % 6) for b in range(B)]
    yk, ik = eng.infer_panel_batch_infer(xd, None, pd, bd, rng_keys=keys, **kw)
    for b, (s, j) in enumerate(keys):
        # the same input at row j of a uniform batch with seed s (rows in front of it: copies of other rows' texts)
        rows = [(b + 1 + k) % B for k in range(j)] + [b]
        yu, iu = eng.infer_panel_batch_infer([xd[r] for r in rows], None, pd[b].unsqueeze(0).expand(j + 1, -1).contiguous(),
                                             [bd[r] for r in rows], seed=s, **kw)
        assert iu[j] == ik[b] and yu[j].tolist() == yk[b].tolist(), f"row {b} keyed {(s, j)} draws differently"
    # the keys are what separates the rows: without them the draws follow (seed, row in the launch)
    assert len({tuple(y.tolist()) for y in yk}) == B
    # no keys = keys (seed, b): the draws of a batch without keys are unchanged
    y0, i0 = eng.infer_panel_batch_infer(xd, None, pd, bd, seed=77, **kw)
    y1, i1 = eng.infer_panel_batch_infer(xd, None, pd, bd, seed=0, rng_keys=[(77, b) for b in range(B)], **kw)
    assert i0 == i1 and [y.tolist() for y in y0] == [y.tolist() for y in y1]
    y2, _ = eng.infer_panel_batch_infer(xd, None, pd, bd, seed=78, **kw)
    assert [y.tolist() for y in y2] != [y.tolist() for y in y0], "the seed must matter"
