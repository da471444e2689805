"""CPU: the host mirrors of the alignment kernels (tests/_align_ref.py) are themselves right -- the float64 search finds the maximal
monotonic path and, among maximal ones, the one VITS' tie rule selects (against a brute force over every path for nf <= 7,
nl <= 4); a planted alignment is recovered exactly; the fallback; and the header / binding of the new entry points."""
import os
import re

import numpy as np
import pytest

import _align_ref as R
from conftest import ROOT
from gsv.timestamps import build_marks, to_json, total_seconds      # the mirrors below are what the device tests and these stand on


def _cases():
    rng = np.random.default_rng(7)
    for nf in range(1, 8):
        for nl in range(1, min(nf, 4) + 1):
            yield nf, nl, "const", np.full((nf, nl), -1.0, np.float32)
            yield nf, nl, "quant4", -rng.integers(0, 4, (nf, nl)).astype(np.float32)
            yield nf, nl, "quant4b", -rng.integers(0, 4, (nf, nl)).astype(np.float32) * 0.25
            yield nf, nl, "dyadic", -rng.integers(0, 1 << 12, (nf, nl)).astype(np.float32) / 256.0


def test_mirror_equals_brute_force_over_every_monotonic_path():
    n = 0
    for nf, nl, name, lp in _cases():
        ends, score, V = R.dp_mirror(lp)
        want, total = R.brute_force(lp)
        assert R.path_sum(lp, ends) == total == V[nl - 1], (nf, nl, name)
        assert ends.tolist() == want.tolist(), (nf, nl, name, lp)
        assert score == np.float32(total / nf)
        n += 1
    assert n == 4 * sum(min(nf, 4) for nf in range(1, 8))


def test_a_tie_stays():
    # two frames more than phonemes, all cells equal: every path ties; walking back, the rule stays on the last phoneme as long
    # as it may, so the extra frames go to the LAST phoneme
    ends, score, _ = R.dp_mirror(np.zeros((5, 3), np.float32))
    assert ends.tolist() == [1, 2, 5] and score == 0.0


def test_random_float_paths_are_maximal():
    rng = np.random.default_rng(3)
    for nf, nl in [(7, 4), (6, 3), (7, 2), (5, 5)]:
        lp = np.log(rng.dirichlet(np.ones(nl), nf)).astype(np.float32)
        ends, _, V = R.dp_mirror(lp)
        best = max(R.path_sum(lp, e) for e in R.all_paths(nf, nl))
        assert abs(R.path_sum(lp, ends) - best) <= 1e-12 and abs(V[nl - 1] - best) <= 1e-12


@pytest.mark.parametrize("nf,nl", [(400, 57), (131, 100), (64, 64), (9, 1)])
def test_planted_alignment_is_recovered(nf, nl):
    q, k, scale, ends = R.planted(nf, nl, 4, 128, seed=nf)
    lp, a_max, s_max = R.logp_mirror(q, k, 4, scale)
    path = R.path_of(ends, nf)
    on = lp[np.arange(nf), path]
    off = np.where(np.arange(nl)[None, :] == path[:, None], -np.inf, lp)
    if nl > 1:
        assert (on - off.max(axis=1)).min() > 1.0, "the true path wins every row by more than 1"
    got, score, _ = R.dp_mirror(lp.astype(np.float32))
    assert got.tolist() == ends.tolist()
    assert a_max == 4.0 and s_max == 4.0 * scale


def test_fallback():
    assert R.fallback_ends(3, 5).tolist() == [0, 1, 1, 2, 3]
    assert R.fallback_ends(10, 4).tolist() == [2, 5, 7, 10]
    ends, score, V = R.dp_mirror(np.zeros((3, 5), np.float32))
    assert ends.tolist() == [0, 1, 1, 2, 3] and score == -np.inf and V is None
    assert not R.searched(1025, 1025) and R.searched(1024, 1024) and not R.searched(0, 0)


def test_logp_mirror_is_a_renormalised_mean_of_softmaxes():
    rng = np.random.default_rng(0)
    q, k = rng.standard_normal((5, 8)), rng.standard_normal((3, 8))
    lp, a_max, s_max = R.logp_mirror(q, k, 2, 0.5)
    assert np.allclose(np.exp(lp).sum(axis=1), 1.0, atol=1e-12)
    s0 = 0.5 * q[:, :4] @ k[:, :4].T
    s1 = 0.5 * q[:, 4:] @ k[:, 4:].T
    sm = lambda s: np.exp(s) / np.exp(s).sum(axis=1, keepdims=True)
    assert np.allclose(lp, np.log((sm(s0) + sm(s1)) / 2), atol=1e-12)
    bar = R.logp_bar(lp, a_max, s_max, 2, 4, 0.5)
    assert bar.shape == lp.shape and (bar > 0).all() and bar.max() < 1e-4


def test_header_and_binding_carry_the_entry_points():
    from gsv import _lib
    hdr = open(os.path.join(ROOT, "include", "gsv.h")).read()
    for name in ("gsv_op_align_workspace", "gsv_op_align_logp", "gsv_op_align_path", "gsv_op_align", "gsv_vits_set_align"):
        assert re.search(r"\b%s\(" % name, hdr) and name in _lib.EXPORTS
    import ctypes
    assert ctypes.sizeof(_lib.AlignSpan) == 24 and ctypes.sizeof(_lib.AlignSegSpan) == 20
    assert np.dtype(_lib.ALIGN_SPAN_DTYPE).itemsize == 24


# ---- gsv.timestamps.build_marks (pure host code) ----

def _sent(n_samples, nf=None, ends=None, phones=None, **kw):
    s = dict(n_samples=n_samples, **kw)
    if ends is not None:
        s.update(nf=nf, ends=np.asarray(ends, np.int32), phones=phones if phones is not None else list(range(100, 100 + len(ends))),
                 score=kw.get("score", -1.5))
    return s


@pytest.mark.parametrize("gap_s", [0.0, 0.3])
def test_build_marks_offsets_order_and_total_length(gap_s):
    sr, up = 32000, 640
    gap = int(sr * gap_s)
    # three sentences as two buckets emit them: bucket 0 holds sentences 2 and 0, bucket 1 sentence 1; an empty sentence last
    sents = [_sent(10 * up, 10, [3, 4, 10], text="a"), _sent(6 * up, 6, [1, 6], text="b"), _sent(4 * up, 4, [4], text="c"),
             _sent(0, text="")]
    marks = build_marks(sents, sr, gap, order=[2, 0, 1, 3])
    assert [m["index"] for m in marks] == [2, 0, 1, 3] and [m["text"] for m in marks] == ["c", "a", "b", ""]
    off = 0.0
    for m, s in zip(marks, [sents[i] for i in (2, 0, 1, 3)]):
        assert abs(m["start"] - off) < 1e-12 and abs(m["end"] - off - s["n_samples"] / sr) < 1e-12
        off += (s["n_samples"] + gap) / sr
        if m["phones"]:
            assert m["phones"][0][1] == m["start"] and abs(m["phones"][-1][2] - m["end"]) < 1e-12
            assert all(a[2] == b[1] for a, b in zip(m["phones"], m["phones"][1:])), "a phoneme starts where the last one ends"
    audio_len = sum(s["n_samples"] + gap for s in sents)
    assert abs(total_seconds(marks, sr, gap) - audio_len / sr) < 1e-9, "the last sentence's end + gap is len(audio) / sr"
    # exact at speed 1: a frame is `up` samples
    a = marks[1]
    assert [round((p[2] - a["start"]) * sr) for p in a["phones"]] == [3 * up, 4 * up, 10 * up]
    assert [p[0] for p in a["phones"]] == [100, 101, 102] and a["confidence"] == -1.5
    assert marks[3]["phones"] == [] and marks[3]["start"] == marks[3]["end"] and marks[3]["confidence"] is None


def test_build_marks_is_proportional_at_another_speed_and_keeps_fallback_spans():
    sr = 32000
    # speed 1.25: 10 pre-speed frames came out as 9 frames of 640 samples
    m, = build_marks([_sent(9 * 640, 10, [5, 10])], sr, 0)
    assert abs(m["phones"][0][2] - 0.5 * 9 * 640 / sr) < 1e-12 and abs(m["phones"][1][2] - m["end"]) < 1e-12
    # the AR stopped early: 3 frames for 5 phonemes, proportional ends with empty phonemes, confidence -inf
    fb = R.fallback_ends(3, 5)
    m, = build_marks([_sent(3 * 640, 3, fb, score=float("-inf"))], sr, 0, offset=2.0)
    assert m["confidence"] == -np.inf and m["start"] == 2.0
    assert [p[2] >= p[1] for p in m["phones"]] == [True] * 5 and m["phones"][0][1] == m["phones"][0][2], "an empty phoneme"
    assert to_json([m])[0]["confidence"] is None and isinstance(to_json([m])[0]["phones"][0], list)
    # "sentence" mode: no ends at all
    m, = build_marks([dict(n_samples=100, text="x", index=7)], sr, 10)
    assert m == {"index": 7, "text": "x", "start": 0.0, "end": 100 / sr, "confidence": None, "phones": []}


def test_build_marks_units_from_word2ph_and_bad_input():
    sr = 32000
    s = _sent(8 * 640, 8, [1, 3, 4, 6, 8], text="你好，吗", word2ph=[2, 2, 0, 1])
    m, = build_marks([s], sr, 0)
    u = m["units"]
    assert [x[0] for x in u] == list("你好，吗")
    assert u[0][1] == m["start"] and u[0][2] == m["phones"][1][2] and u[1][2] == m["phones"][3][2]
    assert u[2][1] == u[2][2] == u[1][2], "a character without phonemes is an instant"
    assert abs(u[3][2] - m["end"]) < 1e-12
    for bad in (dict(word2ph=[2, 2, 1]), dict(word2ph=[2, 2, 0, 2])):
        with pytest.raises(ValueError):
            build_marks([dict(s, **bad)], sr, 0)
    with pytest.raises(ValueError):
        build_marks([_sent(640, 2, [2, 1])], sr, 0)
    with pytest.raises(ValueError):
        build_marks([_sent(640, 2, [1, 2])], sr, 0, order=[0, 0])
    with pytest.raises(ValueError):
        build_marks([_sent(640, 2, [1, 3])], sr, 0)


def test_the_pre_processor_keeps_word2ph_for_whole_zh_sentences():
    from gsv.TTS_infer_pack.TextPreprocessor import sentence_word2ph
    assert sentence_word2ph([[2, 2], [0, 1]], [1] * 5, "你好，吗") == [2, 2, 0, 1]
    assert sentence_word2ph([[2, 2], None], [1] * 6, "你好ab") is None, "a run without word2ph (en): no units for the sentence"
    assert sentence_word2ph([[2, 2]], [1] * 5, "你好") is None and sentence_word2ph([[2, 2]], [1] * 4, "你好吗") is None
    assert sentence_word2ph([], [], "") is None
    m, = build_marks([_sent(4 * 640, 4, [1, 2, 3, 4], text="你好", word2ph=sentence_word2ph([[2, 2]], [1] * 4, "你好"))], 32000, 0)
    assert [u[0] for u in m["units"]] == ["你", "好"]
