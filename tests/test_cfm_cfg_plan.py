"""CPU: TTS.plan_cfm with the request key `inference_cfg_rate` -- guided and unguided requests and different rates take
separate passes, a guided pass holds at most cfm_max_rows // 2 request rows (each brings its unconditioned twin), unguided
plans are what they were -- plus the option plumbing and the C ABI of the guided entry.  No compute is called here."""
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT
from gsv.TTS_infer_pack.TTS import TTS
from test_run_batch_cfm_plan import VC, _plan, _reference_cuts, _stub


def _n(T_min, frames):
    return len(_reference_cuts(frames, VC["T_chunk"] - T_min, VC["overlapped_len"]))


def test_request_option_and_keywords():
    assert TTS._request_options({})["inference_cfg_rate"] == 0
    assert TTS._request_options({"inference_cfg_rate": 0.7})["inference_cfg_rate"] == 0.7
    for fn in (TTS.using_vocoder_synthesis, TTS.using_vocoder_synthesis_batched_infer):
        assert inspect.signature(fn).parameters["inference_cfg_rate"].default == 0, fn.__name__
    # _synthesize_batch hands the resolved options on: rate, steps, speed, and the seed of the batch / of each chunked sentence
    calls = []
    stub = SimpleNamespace(configs=SimpleNamespace(use_vocoder=True, device="cpu"),
                           using_vocoder_synthesis_batched_infer=lambda idx, sem, ph, **kw: calls.append(kw) or [None] * len(idx),
                           using_vocoder_synthesis=lambda sem, ph, **kw: calls.append(kw))
    item = {"phones": [torch.arange(3), torch.arange(4)]}
    pred_list, idx_list = [torch.arange(9), torch.arange(7)], [5, 2]
    actual_seed, bi = 100, 3
    for req, (rate, steps, speed) in (({}, (0, 32, 1.0)),
                                      ({"inference_cfg_rate": 0.7, "sample_steps": 8, "speed_factor": 1.25}, (0.7, 8, 1.25))):
        for parallel in (True, False):
            del calls[:]
            opts = TTS._request_options(dict(req, parallel_infer=parallel))
            TTS._synthesize_batch(stub, item, [p[-i:] for p, i in zip(pred_list, idx_list)], pred_list, idx_list, bi, actual_seed,
                                  opts, ([], {}))
            assert len(calls) == (1 if parallel else len(idx_list))
            assert all((kw["inference_cfg_rate"], kw["sample_steps"], kw["speed"]) == (rate, steps, speed) for kw in calls)
            assert [kw["seed"] for kw in calls] == ([actual_seed + bi] if parallel else
                                                    [actual_seed + bi * 4096 + k for k in range(len(idx_list))])
    from gsv.module.models import CFM
    assert inspect.signature(CFM.inference_rows).parameters["inference_cfg_rate"].default == 0
    assert inspect.signature(CFM.inference).parameters["inference_cfg_rate"].default == 0
    assert list(inspect.signature(CFM.inference_guided).parameters) == list(inspect.signature(CFM.inference).parameters)


def test_guided_unguided_and_different_rates_take_separate_passes():
    plans = [_plan(14, [150], inference_cfg_rate=0.7),
             _plan(20, [90]),                                           # unguided
             _plan(17, [100], inference_cfg_rate=0.7),                  # joins request 0's group: another voice, the same rate
             _plan(14, [60], inference_cfg_rate=2.0),                   # another rate
             _plan(20, [40], inference_cfg_rate=1e-6),                  # at or below 1e-5: unguided, with request 1
             _plan(20, [40], inference_cfg_rate=-1.0),                  # negative: unguided
             _plan(14, [70], inference_cfg_rate=0.7, sample_steps=8),   # steps still split
             _plan(20, [60], inference_cfg_rate=0.7, parallel_infer=False)]   # chunk by chunk: not shared
    fold = lambda r, T_min, frames: [(r, 0, k) for k in range(_n(T_min, frames))]
    g07 = fold(0, 14, 150) + fold(2, 17, 100)
    plain = fold(1, 20, 90) + fold(4, 20, 40) + fold(5, 20, 40)
    g20 = fold(3, 14, 60)
    g07s8 = fold(6, 14, 70)
    assert TTS.plan_cfm(_stub(10 ** 6), plans) == [g07, plain, g20, g07s8]
    for p in TTS.plan_cfm(_stub(3), plans):
        rates = {plans[r]["opts"]["inference_cfg_rate"] if plans[r]["opts"]["inference_cfg_rate"] > 1e-5 else 0 for r, _, _ in p}
        assert len(rates) == 1 and len({plans[r]["opts"]["sample_steps"] for r, _, _ in p}) == 1


@pytest.mark.parametrize("cap", [1, 2, 3, 7, 8, 32])
def test_a_guided_pass_holds_half_the_rows(cap):
    """cfm_max_rows bounds the DiT rows of a pass: a guided pass takes cap // 2 request rows (1 when cap is 1: a pass cannot
    be empty), an unguided one cap, as before; nothing is lost or doubled, order is kept"""
    plans = [_plan(14, [150, 40], inference_cfg_rate=0.7), _plan(20, [90]), _plan(20, [120], inference_cfg_rate=0.7)]
    guided = [(0, 0, k) for k in range(_n(14, 150))] + [(0, 1, k) for k in range(_n(14, 40))] + [(2, 0, k) for k in range(_n(20, 120))]
    plain = [(1, 0, k) for k in range(_n(20, 90))]
    passes = TTS.plan_cfm(_stub(cap), plans)
    gp = [p for p in passes if plans[p[0][0]]["opts"]["inference_cfg_rate"] > 1e-5]
    up = [p for p in passes if p not in gp]
    half = max(1, cap // 2)
    assert all(1 <= len(p) <= half for p in gp) and all(1 <= len(p) <= cap for p in up)
    assert all(len(p) == half for p in gp[:-1]) and all(len(p) == cap for p in up[:-1])
    assert [e for p in gp for e in p] == guided and [e for p in up for e in p] == plain
    if cap >= 2:
        assert all(2 * len(p) <= cap for p in gp), "a guided pass runs the DiT over 2 x its rows"


def test_unguided_plans_are_what_they_were():
    """without the key, with 0 and with a rate below the threshold: the passes of test_what_is_shared_grouping_and_caps"""
    def plans(**kw):
        return [_plan(14, [150, 40], **kw), _plan(20, [60], parallel_infer=False, **kw), _plan(20, [0, 90], speed_factor=1.25, **kw),
                _plan(17, [100], sample_steps=8, **kw), _plan(20, [], **kw)]
    rows32 = [(0, 0, k) for k in range(_n(14, 150))] + [(0, 1, k) for k in range(_n(14, 40))] + [(2, 1, k) for k in range(_n(20, 90))]
    rows8 = [(3, 0, k) for k in range(_n(17, 100))]
    for kw in ({}, {"inference_cfg_rate": 0}, {"inference_cfg_rate": 1e-6}):
        assert TTS.plan_cfm(_stub(10 ** 6), plans(**kw)) == [rows32, rows8]
        for cap in (3, len(rows32) - 1, len(rows32)):
            want = [rows[i:i + cap] for rows in (rows32, rows8) for i in range(0, len(rows), cap)]
            assert TTS.plan_cfm(_stub(cap), plans(**kw)) == want
    # plans made before the key existed (no "inference_cfg_rate" among the options) still plan
    old = plans()
    for pl in old:
        del pl["opts"]["inference_cfg_rate"]
    assert TTS.plan_cfm(_stub(10 ** 6), old) == [rows32, rows8]
    assert TTS.plan_cfm(_stub(32, use_vocoder=False), plans(inference_cfg_rate=0.7)) == []


def test_library_exports_the_guided_entry_and_the_header_declares_it():
    from gsv import build, _lib
    build.build(verbose=False)
    assert hasattr(_lib.lib(), "gsv_cfm_inference_guided")
    assert "gsv_cfm_inference_guided" in _lib.EXPORTS
    src = open(os.path.join(ROOT, "include", "gsv.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+gsv_cfm_inference_guided\s*\(([^)]*)\)", src)
    assert m and re.search(r"float\s+temperature\s*,\s*float\s+cfg_rate\s*,\s*float\s*\*\s*out", m.group(1))
    # the two unguided entries keep their signatures
    assert re.search(r"\bint\s+gsv_cfm_inference_rows\s*\([^)]*float\s+temperature\s*,\s*float\s*\*\s*out\s*,\s*gsv_stream_t\s+stream\s*\)", src)
    assert re.search(r"\bint\s+gsv_cfm_inference\s*\([^)]*uint64_t\s+seed\s*,\s*float\s*\*\s*out\s*,\s*gsv_stream_t\s+stream\s*\)", src)
