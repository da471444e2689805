"""GPU: TTS.run_batch(continuous_ar=True) -- each plan_batch group decoded through one AR decode session instead of launches of
max_batch rows -- against run_batch() on the fp32 small v2 pipeline: the same tokens per sentence, audio within 1 int16 LSB
(the project's bar for run_batch against run)."""
import numpy as np
import pytest

from test_run_batch_gpu import _build, _segs, _voice_args
from test_run_batch_shared_gpu import BASE, _lsb

pytestmark = pytest.mark.gpu


def _requests(mixed):
    """6 requests, 3 voices, 2 to 5 sentences each: 19 sentences for the 4 slots of the fixture's decoder"""
    va, vb, vc = _voice_args(0, 8, 6, "v2"), _voice_args(1, 23, 4, "v2"), _voice_args(2, 5, 7, "v2")
    other = dict(BASE, top_k=12, top_p=0.9, temperature=0.8, repetition_penalty=1.2) if mixed else BASE
    return [
        (va, dict(BASE, segments=_segs(30, [9, 5]), seed=3)),
        (vb, dict(other, segments=_segs(31, [7, 12, 6]), batch_size=2, seed=4)),
        (vc, dict(BASE, segments=_segs(32, [11, 6, 8, 5, 10]), batch_size=5, seed=5)),
        (va, dict(other, segments=_segs(33, [6, 9, 7, 8]), batch_size=3, seed=6)),
        (vb, dict(BASE, segments=_segs(34, [10, 4]), seed=7)),
        (vc, dict(other, segments=_segs(35, [8, 7, 13]), batch_size=2, seed=8)),
    ]


def _run_batch(tts, batch, **kw):
    """run_batch's output and the AR stage's tokens per (request, to_batch batch, sentence)"""
    seen = []
    stage = tts._ar_stage

    def spy(plans, **k):
        stage(plans, **k)
        seen.append([[[p.cpu().tolist() for p in pred] for pred in pl["preds"]] for pl in plans])
    tts._ar_stage = spy
    try:
        out = tts.run_batch(batch, **kw)
    finally:
        del tts._ar_stage
    return out, seen[-1]


@pytest.fixture(scope="module")
def tts():
    return _build("v2")


@pytest.mark.parametrize("mixed", [False, True])
def test_continuous_ar_equals_static_launches(tts, mixed):
    reqs = _requests(mixed)
    assert sorted(len(r["segments"]) for _, r in reqs) == [2, 2, 3, 3, 4, 5]
    voices = {}
    for kw, _ in reqs:
        voices.setdefault(id(kw), tts.make_voice(**kw))
    batch = [dict(req, voice=voices[id(kw)]) for kw, req in reqs]
    plain, preds_plain = _run_batch(tts, batch, mixed_sampling=mixed)
    sessions = []
    inner = tts.t2s_model.infer_panel_continuous

    def spy(x, *a, **k):
        out = inner(x, *a, **k)
        sessions.append((len(x), k.get("row_sampling") is not None, tts.t2s_model.last_session))
        return out
    tts.t2s_model.infer_panel_continuous = spy
    try:
        cont, preds_cont = _run_batch(tts, batch, mixed_sampling=mixed, continuous_ar=True)
    finally:
        del tts.t2s_model.infer_panel_continuous
    # one group (one sampling setting, or mixed_sampling over two): one session for all 19 sentences
    assert [n for n, _, _ in sessions] == [19]
    assert all(per_row == mixed for _, per_row, _ in sessions)
    for n, _, ses in sessions:
        assert ses.slots == 4 and len(ses.history) == n and len(ses.adopt) >= 2, "the queue must exceed the slots"
    assert preds_cont == preds_plain, "a sentence decodes other tokens in a session"
    assert len({tuple(p) for pl in preds_cont for pred in pl for p in pred}) == 19
    for r, ((sr_a, a), (sr_b, b)) in enumerate(zip(plain, cont)):
        assert sr_a == sr_b and a.dtype == b.dtype == np.int16 and a.shape == b.shape
        assert _lsb(a, b) <= 1, f"request {r}: continuous_ar differs by {_lsb(a, b)} LSB"
        assert np.abs(a).max() > 0
