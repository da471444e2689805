"""CPU: TextPreprocessor.preprocess_many -- many requests' texts, the zh BERT features of all of them from one `bert_fn.batch`
call -- returns exactly what `preprocess` returns per request.  A fake `bert_fn` stands in for the engine: a deterministic
vector per (character, position in its text), every call recorded."""
import pytest
import torch


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


def _vec(text):
    col = torch.arange(1024, dtype=torch.float32) * 1e-3
    return torch.stack([col + float(ord(ch) % 997) + 0.01 * i for i, ch in enumerate(text)]) if text else torch.zeros(0, 1024)


class _FakeBert:
    def __init__(self):
        self.calls, self.batches = [], []

    def __call__(self, text):
        self.calls.append(text)
        return _vec(text)

    def batch(self, texts):
        self.batches.append(list(texts))
        return [_vec(t) for t in texts]


class _FakeBertNoBatch:
    def __init__(self):
        self.calls = []

    def __call__(self, text):
        self.calls.append(text)
        return _vec(text)


LONG = "今天天气不错，" * 90                                      # 630 characters without a sentence end: split_big_text cuts it
ITEMS = [
    ("你好，我是小明。今天天气不错，我们一起去公园散步吧！", "all_zh", "cut5"),
    ("HH AH0 L OW1 W ER1 L D . DH IH1 S IH1 Z AH0 T EH1 S T !", "en", "cut4"),
    ("你好，我是HH AH0 L OW1小明，今天天气不错。", "zh", "cut0"),
    ("嗯！", "all_zh", "cut0"),
    (LONG, "all_zh", "cut0"),
]


@pytest.fixture(scope="module")
def backends():
    from gsv.text import cleaner, g2p
    cleaner.register_g2p("zh", _ToyZh())
    cleaner.register_g2p("en", g2p.SymbolG2P())


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["phones"] == y["phones"] and x["norm_text"] == y["norm_text"]
        assert x["bert_features"].shape == y["bert_features"].shape == (1024, len(x["phones"]))
        assert x["bert_features"].dtype == y["bert_features"].dtype and torch.equal(x["bert_features"], y["bert_features"])


def test_preprocess_many_equals_preprocess_per_item(backends):
    from gsv.TTS_infer_pack.TextPreprocessor import TextPreprocessor
    one, many = _FakeBert(), _FakeBert()
    ref = [TextPreprocessor(bert_fn=one).preprocess(*it, "v2") for it in ITEMS]
    out = TextPreprocessor(bert_fn=many).preprocess_many(ITEMS, "v2")
    assert len(out) == len(ITEMS)
    for a, b in zip(out, ref):
        _same(a, b)
    # the cases the list is there for
    assert not bool(ref[1][0]["bert_features"].any())                                 # en: zero features
    assert "HH AH0 L OW1" in ref[2][0]["norm_text"] and bool(ref[2][0]["bert_features"].any())   # zh + en runs in one sentence
    assert len(ref[3]) == 1 and len(ref[3][0]["norm_text"]) == 4 and ref[3][0]["norm_text"].startswith(".")   # 3 characters: retried
    assert len(ref[4]) > 1 and all(len(s["norm_text"]) <= 510 for s in ref[4])        # cut by split_big_text
    # one batch call, no per-text call, the zh runs in order.  preprocess also calls bert_fn for the attempt that the
    # short-sentence retry throws away; preprocess_many retries on the phones and never computes those features
    assert many.calls == [] and len(many.batches) == 1
    kept = [t for t in one.calls if t != "。嗯！"]
    assert many.batches[0] == kept and len(one.calls) == len(kept) + 1


def test_bert_fn_without_batch_is_called_per_text(backends):
    from gsv.TTS_infer_pack.TextPreprocessor import TextPreprocessor
    plain = _FakeBertNoBatch()
    out = TextPreprocessor(bert_fn=plain).preprocess_many(ITEMS[:1] + ITEMS[2:3], "v2")
    ref_fn = _FakeBert()
    ref = [TextPreprocessor(bert_fn=ref_fn).preprocess(*it, "v2") for it in ITEMS[:1] + ITEMS[2:3]]
    for a, b in zip(out, ref):
        _same(a, b)
    assert plain.calls == ref_fn.calls and len(plain.calls) >= 3


def test_no_zh_text_makes_no_batch_call(backends):
    from gsv.TTS_infer_pack.TextPreprocessor import TextPreprocessor
    fake = _FakeBert()
    tp = TextPreprocessor(bert_fn=fake)
    out = tp.preprocess_many([ITEMS[1]], "v2")
    _same(out[0], tp.preprocess(*ITEMS[1], "v2"))
    assert fake.batches == [] and fake.calls == []
    assert tp.preprocess_many([], "v2") == [] and fake.batches == []
    # and zh text without a BERT back-end is refused as preprocess refuses it
    with pytest.raises(NotImplementedError):
        TextPreprocessor().preprocess_many([ITEMS[0]], "v2")
