"""GPU: the prefill with its GEMMs on the panel kernel (set_prefill_gemm(1)) against the dispatcher (set_prefill_gemm(0)), on a small
synthetic fp16 model (dim 512, 16 heads, 2 layers), greedy for 8 steps: ids, per-step logits and the K/V cache rows j < S_b of both
layers must be byte-identical, and each handle must have taken the kernel it was told to take (route record of the prefill's last
GEMM: family 9 = the panel kernel).

Two batches:
  * B = 3 ragged rows, S up to 130 (M = 278 rows).  Here the dispatcher launches gemm_t64 (csrc/gemm_sk.hip: two accumulators per
    element, even / odd k-steps), and the prefill takes the panel kernel's form with that summation (route p2 = 1).
  * B = 16 rows of S = 131 (M = 2096 rows): from 2049 rows on the dispatcher takes gemm_lds (asserted), and the prefill takes the
    single-accumulator form.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = 8
SMALL = ((41, 17, 30), (89, 100, 1))                    # x_len, p_len: S_b = 130, 117, 31
LARGE = ((41,) * 16, (90,) * 16)                        # S_b = 131, M = 2096


def _run(mode, cfg, sd, xs, berts, prompts):
    from gsv.AR.models.t2s_model import Text2SemanticDecoder
    m = Text2SemanticDecoder(cfg, device=DEV, dtype=torch.float16, max_batch=len(xs), max_seq=192)
    m.load_state_dict(sd)
    m.set_prefill_gemm(mode)
    ys, idx = m.infer_panel_batch_infer([x.to(DEV) for x in xs], None, [p.to(DEV) for p in prompts], [b.to(DEV) for b in berts],
                                        top_k=1, top_p=1.0, temperature=1.0, early_stop_num=STEPS, repetition_penalty=1.35,
                                        dump_logits=True)
    logits = m.last_logits_dump.cpu().numpy()
    kv = [m.debug_kv(layer, which, b, xs[b].numel() + prompts[b].numel()).view(torch.int16).numpy()
          for layer in range(2) for which in range(2) for b in range(len(xs))]
    return [y.cpu().tolist() for y in ys], idx, logits, kv, (m.last_prefill_route & 255, m.last_prefill_route >> 32 & 255)


def _compare(xlens, plens, want_family0, want_sum2):
    from gsv import synthetic as S
    cfg = S.small_t2s_config(n_layer=2, dim=512, head=16)
    sd = S.make_t2s_state_dict(cfg, seed=3, suppress_eos=True)
    mc = cfg["model"]
    xs = [torch.from_numpy(S.hash_ints(f"pg_x{i}", n, mc["phoneme_vocab_size"], 1)).long() for i, n in enumerate(xlens)]
    berts = [S.hash_symmetric(f"pg_bert{i}", (1024, n), 0.5, 1) for i, n in enumerate(xlens)]
    prompts = [torch.from_numpy(S.hash_ints(f"pg_p{i}", n, mc["vocab_size"] - 1, 1)).long() for i, n in enumerate(plens)]
    y0, i0, l0, kv0, (fam0, _) = _run(0, cfg, sd, xs, berts, prompts)
    y1, i1, l1, kv1, (fam1, sum2) = _run(1, cfg, sd, xs, berts, prompts)
    kv_bad = sum(not np.array_equal(a, b) for a, b in zip(kv0, kv1))
    kv_diff = max(float(np.abs(a.view(np.float16).astype(np.float32) - b.view(np.float16).astype(np.float32)).max()) for a, b in zip(kv0, kv1))
    kv_max = max(float(np.abs(a.view(np.float16).astype(np.float32)).max()) for a in kv0)
    print(f"[prefill_gemm] B = {len(xs)}, M = {sum(xlens) + sum(plens)}: families {fam0} / {fam1}; ids equal {y0 == y1 and i0 == i1}; "
          f"logits differing {int((l0.view(np.int32) != l1.view(np.int32)).sum())} of {l0.size}, max |diff| {np.abs(l0 - l1).max():.3e} "
          f"at |logits| <= {np.abs(l0).max():.1f}; K/V blocks differing {kv_bad} of {len(kv0)}, max |diff| {kv_diff:.3e} at |K/V| <= {kv_max:.1f}")
    assert fam1 == 9, f"set_prefill_gemm(1) ran the prefill's last GEMM on family {fam1}, not on the panel kernel"
    assert fam0 not in (0, 9), f"set_prefill_gemm(0) ran the prefill's last GEMM on family {fam0}"
    assert fam0 == want_family0, f"the dispatcher ran family {fam0}, expected {want_family0}"
    assert sum2 == want_sum2, f"the panel kernel ran summation form {sum2}, expected {want_sum2}"
    assert i0 == i1 and y0 == y1, "ids differ"
    assert np.isfinite(l0).all() and l0.shape[1] == len(xs)
    assert np.array_equal(l0.view(np.int32), l1.view(np.int32)), "per-step logits differ"
    assert all(a.shape[1] > 0 for a in kv0) and any(a.any() for a in kv0), "the K/V rows read back are empty"
    assert kv_bad == 0, "K/V cache rows differ"


def test_prefill_on_the_panel_gemm_is_bit_identical_to_the_dispatcher():
    _compare(*SMALL, want_family0=2, want_sum2=1)


def test_prefill_on_the_panel_gemm_is_bit_identical_where_the_dispatcher_takes_gemm_lds():
    _compare(*LARGE, want_family0=4, want_sum2=0)
