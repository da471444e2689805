"""CPU: TTS.plan_vocoder -- which v3 / v4 folds run_batch(shared_cfm=True, shared_vocoder=True) vocodes together, in which
order, and where a pass ends.  No compute is called here."""
import inspect
from types import SimpleNamespace

import pytest

from gsv.TTS_infer_pack.TTS import TTS

VC = {"T_ref": 20, "T_chunk": 48, "overlapped_len": 4, "upsample_rate": 256, "sr": 24000}


def _stub(max_frames, use_vocoder=True, vc=VC):
    return SimpleNamespace(configs=SimpleNamespace(use_vocoder=use_vocoder), vocoder_configs=dict(vc), vocoder_max_frames=max_frames,
                           _chunk_cuts=TTS._chunk_cuts)


def _plan(T_min, folds, **opts):
    return dict(T_min=T_min, cfm_folds=list(folds), opts=TTS._request_options(opts))


def _mel_frames(T_min, frames):
    """chunks x chunk_len of the fold's voice: what _fold_mel hands the vocoder"""
    chunk_len = VC["T_chunk"] - T_min
    return len(TTS._chunk_cuts(frames, chunk_len, VC["overlapped_len"])) * chunk_len


PLANS = [_plan(14, [150, 40]),                         # two to_batch batches: two folds, chunk_len 34
         _plan(20, [60], parallel_infer=False),        # the chunk-by-chunk path: not shared
         _plan(20, [0, 90], speed_factor=1.25),        # an empty fold is left out; speed does not matter
         _plan(17, [100], sample_steps=8),             # another flow-matching group, the same vocoder
         _plan(20, [])]                                # no text
FOLDS = [(0, 0), (0, 1), (2, 1), (3, 0)]
SIZES = [_mel_frames(14, 150), _mel_frames(14, 40), _mel_frames(20, 90), _mel_frames(17, 100)]


def test_keyword_and_class_attribute():
    p = inspect.signature(TTS.run_batch).parameters
    assert p["shared_vocoder"].default is False and p["shared_cfm"].default is False
    assert isinstance(TTS.vocoder_max_frames, int) and TTS.vocoder_max_frames >= 1
    # the initial cap keeps the gapped layout under 2^24 output rows for both vocoders' rates, a gap per frame being the worst case
    assert TTS.vocoder_max_frames * 480 < (1 << 24)


def test_fold_sizes_are_whole_chunks():
    """150 frames after 4 of left padding in chunks of 34 that overlap by 4: cuts start at 0, 30, ..., 150 -> 6 chunks"""
    assert SIZES[0] == 6 * 34 and all(n % c == 0 for n, c in zip(SIZES, (34, 34, 28, 31)))


def test_order_and_what_is_shared():
    assert TTS.plan_vocoder(_stub(10 ** 6), PLANS) == [FOLDS], "(request, batch) order, one pass"


def test_cap_is_respected():
    total = sum(SIZES)
    assert TTS.plan_vocoder(_stub(total), PLANS) == [FOLDS]
    assert TTS.plan_vocoder(_stub(total - 1), PLANS) == [FOLDS[:3], FOLDS[3:]]
    two = TTS.plan_vocoder(_stub(SIZES[0] + SIZES[1]), PLANS)
    assert two == [FOLDS[:2], FOLDS[2:]]
    for cap in (200, 250, 300, total - 1):
        passes = TTS.plan_vocoder(_stub(cap), PLANS)
        assert [f for p in passes for f in p] == FOLDS, "nothing lost, doubled or reordered"
        for p in passes:
            assert len(p) == 1 or sum(SIZES[FOLDS.index(f)] for f in p) <= cap


def test_an_over_long_fold_is_a_pass_of_its_own():
    a, b, c, d = SIZES
    assert a > b + c and b + c + d > a - 1 >= b + c, "the shapes this test is written for"
    # fold (0, 0) alone is past the cap: a pass of its own, and the folds after it still share
    assert TTS.plan_vocoder(_stub(a - 1), PLANS) == [[(0, 0)], [(0, 1), (2, 1)], [(3, 0)]]
    assert TTS.plan_vocoder(_stub(1), PLANS) == [[f] for f in FOLDS]


def test_the_engine_limit_ends_a_pass_gaps_included():
    """(frames + gaps) * upsample_rate stays below 2^24 whatever vocoder_max_frames says"""
    vc = dict(VC, upsample_rate=(1 << 24) // (SIZES[0] + SIZES[1] + 7))      # two folds and one gap of 7 are exactly the limit
    assert TTS.plan_vocoder(_stub(10 ** 9, vc=vc), PLANS[:1], gap=7) == [[(0, 0)], [(0, 1)]]
    vc = dict(VC, upsample_rate=(1 << 24) // (SIZES[0] + SIZES[1] + 8))      # one frame of room
    assert TTS.plan_vocoder(_stub(10 ** 9, vc=vc), PLANS[:1], gap=7) == [[(0, 0), (0, 1)]]


def test_v2_shares_nothing():
    assert TTS.plan_vocoder(_stub(32768, use_vocoder=False), PLANS) == []


@pytest.mark.parametrize("kw", [dict(), dict(shared_cfm=True)])
def test_nothing_is_shared_when_the_keyword_is_off(kw):
    """run_batch without shared_vocoder never reaches plan_vocoder or forward_segments: the stage is handed shared_vocoder=False"""
    seen = []

    stub = SimpleNamespace(t2s_model=object(), vits_model=object(), configs=SimpleNamespace(use_vocoder=True), stop_flag=False,
                _plan_request=lambda req: req, _ar_stage=lambda plans, mixed_sampling=False: None, _output_sr=lambda: 24000,
                _shared_cfm_stage=lambda plans, shared_vocoder=False: seen.append(shared_vocoder),
                plan_vocoder=lambda *a, **k: seen.append("planned"), _finish_request=lambda pl, sr: (sr, None))
    TTS.run_batch(stub, [{}], **kw)
    assert seen == ([False] if kw else [])


def test_shared_vocoder_without_shared_cfm_is_a_value_error_on_v3_only():
    mk = lambda use_vocoder: SimpleNamespace(
        t2s_model=object(), vits_model=object(), configs=SimpleNamespace(use_vocoder=use_vocoder), stop_flag=False,
        _plan_request=lambda req: req, _ar_stage=lambda plans, mixed_sampling=False: None, _output_sr=lambda: 32000,
        _shared_cfm_stage=lambda plans, shared_vocoder=False: None, _finish_request=lambda pl, sr: (sr, None))
    with pytest.raises(ValueError):
        TTS.run_batch(mk(True), [{}], shared_vocoder=True)
    assert TTS.run_batch(mk(False), [{}], shared_vocoder=True) == [(32000, None)]
    assert TTS.run_batch(mk(True), [{}], shared_cfm=True, shared_vocoder=True) == [(32000, None)]
