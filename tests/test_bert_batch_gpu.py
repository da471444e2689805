"""The packed zh BERT pass: BertFeature.batch (all texts in one [sum T, 1024] matrix, gsv_op_embed_ln + the row-wise GEMM /
LayerNorm launches + gsv_op_flash_attn64_seg) against a torch fp32 mirror of the 22 layers (tests/_bert_ref.py), and the
plumbing above it: TextPreprocessor.preprocess_many on the real engine, TTS.run_batch(shared_bert=True), TTS.batched_bert.

The mirror is pinned on the CPU against tests/golden/bert_large.npz (transformers.BertModel hidden_states[-3]).  Its measured
gap to that golden: relative rms 2.07e-4, max-abs 9.74e-4 (the golden is stored in fp16); the bar below is ten times that."""
import copy

import numpy as np
import pytest
import torch

from conftest import load_golden
from gsv import synthetic as S

import _bert_ref as R

DEV = "cuda:0"
GOLDEN_TEXT = "你好，我是小明。今天天气不错，我们一起去公园散步吧！"
_ZH = [c for c in S.BERT_TEST_VOCAB[5:] if not c.isascii()]


def _text(n, salt):
    """n characters of the test vocabulary, deterministic"""
    return "".join(_ZH[(i * 7 + salt * 13 + i // 5) % len(_ZH)] for i in range(n))


# the golden 26-character string plus 1, 2, 15, 16, 60 and 510 characters (no replacement was needed: see the per-sentence
# engine's figures in test_packed_pass_matches_the_mirror)
TEXTS = [GOLDEN_TEXT] + [_text(n, k) for k, n in enumerate([1, 2, 15, 16, 60, 510])]
REL_BAR, MAX_BAR = 1e-2, 5e-2                 # the bars of test_bert_feature_matches_transformers_model


def _errs(o, ref):
    o, ref = np.asarray(o, dtype=np.float32), np.asarray(ref, dtype=np.float32)
    return float(np.sqrt(((o - ref) ** 2).mean() / (ref ** 2).mean())), float(np.abs(o - ref).max())


@pytest.fixture(scope="module")
def state():
    return S.make_bert_state_dict(seed=0, layers=22)


@pytest.fixture(scope="module")
def mirror(state):
    return [R.bert_features(state, S.BERT_TEST_VOCAB, t).numpy() for t in TEXTS]


@pytest.fixture(scope="module")
def engine(state):
    from gsv.feature_extractor.bert import BertFeature
    return BertFeature(device=DEV, state_dict=state, vocab=S.BERT_TEST_VOCAB)


def test_mirror_matches_transformers_golden(mirror):
    """CPU: the mirror vs transformers.BertModel on the golden text.  Measured relative rms 2.07e-4, max-abs 9.74e-4."""
    rel, err = _errs(mirror[0], load_golden("bert_large")["feature"])
    print(f"[bert_ref] mirror vs golden: relative rms {rel:.3e}, max-abs {err:.3e}")
    assert rel <= 2.07e-3 and err <= 9.74e-3


@pytest.mark.gpu
def test_packed_pass_matches_the_mirror(engine, mirror):
    """All seven texts in one batch() call against the mirror, bars relative rms <= 1e-2 and max-abs <= 5e-2 per text.  Measured
    on an MI355X over the seven texts: packed pass relative rms 1.41e-3 .. 2.35e-3, max-abs 5.96e-3 .. 7.65e-3; per-sentence
    engine 1.39e-3 .. 2.16e-3, 6.45e-3 .. 9.14e-3 (worst on the 1-character text); golden text vs transformers 1.54e-3, 5.86e-3."""
    p0 = engine.passes
    out = engine.batch(TEXTS)
    assert engine.passes == p0 + 1
    assert len(out) == len(TEXTS)
    for t, o, ref in zip(TEXTS, out, mirror):
        assert tuple(o.shape) == (len(t), 1024) and o.dtype == torch.float32
        rel_b, err_b = _errs(o.cpu().numpy(), ref)
        rel_s, err_s = _errs(engine(t).cpu().numpy(), ref)
        print(f"[bert_batch] {len(t):3d} characters: packed rel rms {rel_b:.3e} max-abs {err_b:.3e} | "
              f"per-sentence rel rms {rel_s:.3e} max-abs {err_s:.3e}")
        assert rel_s <= REL_BAR and err_s <= MAX_BAR, "the per-sentence engine misses the bar on this text: replace the text"
        assert rel_b <= REL_BAR and err_b <= MAX_BAR
    rel, err = _errs(out[0].cpu().numpy(), load_golden("bert_large")["feature"])
    print(f"[bert_batch] golden text vs transformers: relative rms {rel:.3e}, max-abs {err:.3e}")
    assert rel <= REL_BAR and err <= MAX_BAR
    # max_tokens = 512: 28 + 3 + 4 + 17 + 18 + 62 tokens fit one pass, the 512-token text takes its own; order unchanged
    p0 = engine.passes
    out2 = engine.batch(TEXTS, max_tokens=512)
    assert engine.passes == p0 + 2
    for t, o, ref in zip(TEXTS, out2, mirror):
        rel_b, err_b = _errs(o.cpu().numpy(), ref)
        assert tuple(o.shape) == (len(t), 1024) and rel_b <= REL_BAR and err_b <= MAX_BAR
    p0 = engine.passes
    assert engine.batch([]) == [] and engine.passes == p0
    with pytest.raises(ValueError):
        engine.batch(["好" * 511])
    with pytest.raises(ValueError):
        engine.batch(TEXTS[:2], max_tokens=511)
    assert engine.passes == p0


class _ToyZh:                                                    # the toy zh G2P of test_frontend_gpu.py
    def text_normalize(self, t):
        return t

    def g2p(self, norm):
        ph, w2p = [], []
        for ch in norm:
            if ch in "，。！？":
                ph.append({"，": ",", "。": ".", "！": "!", "？": "?"}[ch]); w2p.append(1)
            else:
                ph += ["n", "i3"]; w2p.append(2)
        return ph, w2p


@pytest.fixture(scope="module")
def tts(state):
    from gsv.text import cleaner
    from gsv.TTS_infer_pack.TTS import TTS
    cleaner.register_g2p("zh", _ToyZh())
    tcfg = S.small_t2s_config(n_layer=2, dim=128, head=4, vocab=1025, phoneme_vocab=732)
    tcfg["data"]["max_sec"] = 0.4                           # early_stop_num = 20 tokens
    t = TTS({"device": DEV, "is_half": False, "version": "v2", "max_batch": 4, "max_seq": 256})
    t.init_t2s_weights(state={"weight": S.make_t2s_state_dict(tcfg, seed=11, suppress_eos=False), "config": tcfg})
    vcfg = copy.deepcopy(S.small_vits_config())
    t.init_vits_weights(state={"weight": S.make_vits_state_dict(vcfg, seed=12), "config": vcfg})
    t.init_bert_weights(state_dict=state, vocab=S.BERT_TEST_VOCAB)
    t.set_prompt_cache(prompt_semantic=torch.from_numpy(S.hash_ints("bb_sem", 8, 1024, 7)),
                       refer_spec=[S.make_refer_spec(frames=30, seed=40).to(DEV)],
                       phones=S.hash_ints("bb_ph", 6, 732, 7).tolist(), bert_features=torch.zeros(1024, 6), norm_text="x" * 6)
    return t


ZH_REQUESTS = ["你好，我是小明。今天天气不错！我们一起去公园散步吧。", "这个地上有人在说，我们也要去。可以的！",
               "今天是个好天气。你和我一起去吧！大中国，小公园。"]


@pytest.mark.gpu
def test_preprocess_many_on_the_engine(tts):
    tp = tts.text_preprocessor
    items = [(t, "all_zh", "cut5") for t in ZH_REQUESTS]
    ref = [tp.preprocess(*it, "v2") for it in items]
    p0 = tts.bert_model.passes
    out = tp.preprocess_many(items, "v2")
    assert tts.bert_model.passes == p0 + 1
    assert [len(x) for x in out] == [len(x) for x in ref] and all(len(x) >= 2 for x in ref)
    for a, b in zip(out, ref):
        for x, y in zip(a, b):
            assert x["phones"] == y["phones"] and x["norm_text"] == y["norm_text"]
            assert x["bert_features"].shape == y["bert_features"].shape == (1024, len(x["phones"]))
            # both are within the bars of the mirror; against each other the same bars hold (two fp16 engines, rms 1.0)
            rel, err = _errs(x["bert_features"].numpy(), y["bert_features"].numpy())
            assert rel <= REL_BAR and err <= MAX_BAR


@pytest.mark.gpu
def test_run_batch_shared_bert_makes_one_pass(tts):
    base = dict(top_k=5, top_p=1.0, temperature=1.0, repetition_penalty=1.35, fragment_interval=0.01, text_lang="all_zh",
                text_split_method="cut5")
    reqs = [dict(base, text=t, seed=3 + i) for i, t in enumerate(ZH_REQUESTS)]
    p0 = tts.bert_model.passes
    out = tts.run_batch([dict(r) for r in reqs], shared_bert=True)
    assert tts.bert_model.passes == p0 + 1
    segs = tts.text_preprocessor.preprocess_many([(r["text"], r["text_lang"], r["text_split_method"]) for r in reqs], "v2")
    assert all(len(s) >= 2 for s in segs)
    ref = tts.run_batch([dict(r, segments=s) for r, s in zip(reqs, segs)])
    assert len(out) == len(ref) == 3
    for (sr_a, a), (sr_b, b) in zip(out, ref):
        assert sr_a == sr_b == 32000 and a.dtype == np.int16 and np.abs(a).max() > 0
        assert np.array_equal(a, b), "shared_bert changed more than where the segments come from"
    # requests that bring segments pass through untouched, and an unknown language raises as _segments raises
    p0 = tts.bert_model.passes
    again = tts.run_batch([dict(r, segments=s) for r, s in zip(reqs, segs)], shared_bert=True)
    assert tts.bert_model.passes == p0 and all(np.array_equal(a[1], b[1]) for a, b in zip(again, ref))
    with pytest.raises(ValueError):
        tts.run_batch([dict(reqs[0], text_lang="xx")], shared_bert=True)


@pytest.mark.gpu
def test_run_with_batched_bert_makes_one_pass(tts):
    text = "你好，我是小明。今天天气不错！我们一起去公园散步吧。这个地上有人在说？我们也要一起去公园。"
    req = dict(text=text, text_lang="all_zh", text_split_method="cut5", top_k=5, seed=1, fragment_interval=0.01)
    assert len(tts.text_preprocessor.pre_seg_text(text, "all_zh", "cut5")) == 5
    tts.batched_bert = True
    try:
        p0 = tts.bert_model.passes
        sr, audio = list(tts.run(dict(req)))[-1]
        assert tts.bert_model.passes == p0 + 1
    finally:
        tts.batched_bert = False
    assert sr == 32000 and audio.dtype == np.int16 and audio.size > 0 and np.abs(audio).max() > 0
