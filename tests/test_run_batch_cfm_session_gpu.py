"""GPU: TTS.run_batch(shared_cfm=True, continuous_cfm=True) -- the shared flow-matching stage through one session, requests
with different sample_steps and guidance rates in the same DiT launches -- against run_batch([request]) per request (fp32,
small v3 and v4 pipelines), with the row cap below the mix, and with the keyword off."""
import numpy as np
import pytest

from gsv import synthetic as S
from gsv.module.models import CFMSession
from test_lora_voices_pipeline_gpu import RANK
from test_pipeline_v3_gpu import _build as build_v3
from test_run_batch_cfm_gpu import BAR, BASE, _diff, _spy, _voice
from test_run_batch_gpu import _segs

pytestmark = pytest.mark.gpu
# (rows, prompt lengths) of the inference_rows calls that run_batch(_mix, shared_cfm=True) issues on the commit before
# continuous_cfm existed (small v3 pipeline), recorded there with _spy
PARENT_CALLS = [(6, [14]), (3, [14]), (11, [20]), (3, [17]), (7, [20])]


def _mix(tts, version, vcfg, vsd):
    """three voices, six requests: sample_steps 2 / 3 / 4, rates 0 / 0.7, one parallel_infer=False, one LoRA voice"""
    tts.add_lora_voice("a", state={"weight": S.make_lora_state_dict(vsd, rank=RANK, seed=3), "config": vcfg, "lora_rank": RANK})
    va, vb, vc = (tts.make_voice(**_voice(i, P, n_ph, Tm, version)) for i, (P, n_ph, Tm) in enumerate(((8, 6, 14), (14, 4, 31), (11, 7, 17))))
    return [dict(BASE, voice=va, segments=_segs(20, [9, 5]), batch_size=2, seed=3, sample_steps=2),
            dict(BASE, voice=va, segments=_segs(21, [7]), seed=4, sample_steps=3, inference_cfg_rate=0.7),
            dict(BASE, voice=vb, segments=_segs(22, [11, 6, 8]), batch_size=2, seed=5, sample_steps=4),
            dict(BASE, voice=vc, segments=_segs(23, [6]), parallel_infer=False, seed=6, sample_steps=3),
            dict(BASE, voice=vc, segments=_segs(24, [10]), seed=7, sample_steps=2, inference_cfg_rate=0.7),
            dict(BASE, voice=vb, segments=_segs(25, [8, 6]), batch_size=2, seed=8, sample_steps=3, lora_voice="a")]


def _session_spy(monkeypatch):
    """every CFMSession.admit: (slots, step counts, rates)"""
    seen, inner = [], CFMSession.admit

    def admit(self, mu, prompts, n_timesteps, inference_cfg_rate, **kw):
        slots = inner(self, mu, prompts, n_timesteps, inference_cfg_rate, **kw)
        seen.append((list(slots), list(n_timesteps), list(inference_cfg_rate)))
        return slots
    monkeypatch.setattr(CFMSession, "admit", admit)
    return seen


def _same(one, two, what):
    for r, ((sr_a, a), (sr_b, b)) in enumerate(zip(one, two)):
        assert sr_a == sr_b and a.dtype == b.dtype == np.int16 and a.shape == b.shape, f"request {r}: {a.shape} vs {b.shape}"
        d = _diff(a, b)
        print(f"request {r}: max |{what}| = {d:.3e} of full scale over {a.size} samples")
        assert d <= BAR, f"request {r}: {what} = {d:.3e} of full scale"
        assert np.abs(a).max() > 0


@pytest.mark.parametrize("version", ["v3", "v4"])
def test_mixed_settings_share_one_session(version, monkeypatch):
    """Every request of the mix through run_batch(shared_cfm=True, continuous_cfm=True) against run_batch([request]) alone:
    equal int16 shapes, samples within 5e-3 of full scale, the non-parallel request bit-equal.  One session takes rows of all
    three step counts and both rates, and no one-shot pass runs.  Then the row cap below the mix's DiT rows: every output
    within the same bar of the uncapped result, and at least one slot is admitted into twice (a refill)."""
    tts, _, (vcfg, vsd, _), _ = build_v3(version)
    batch = _mix(tts, version, vcfg, vsd)
    alone = [tts.run_batch([dict(req)])[0] for req in batch]
    tts.cfm_max_rows = 64            # the mix is 30 rows and 6 twins (v4: 31 and 7): uncapped first
    seen, calls = _session_spy(monkeypatch), _spy(tts)
    out = tts.run_batch(batch, shared_cfm=True, continuous_cfm=True)
    assert calls == [], f"continuous_cfm runs no one-shot pass for the shared folds, got {calls}"
    assert len(seen) == 1, f"the mix fits 64 DiT rows: one admission, got {seen}"
    slots, steps, rates = seen[0]
    assert sorted(set(steps)) == [2, 3, 4] and sorted(set(rates)) == [0.0, pytest.approx(0.7)]
    _same(alone, out, "session - alone")
    assert np.array_equal(out[3][1], alone[3][1]), "the parallel_infer=False request takes the per-request path: bit-equal"
    dit_rows = sum(2 if r > 0 else 1 for r in rates)
    tts.cfm_max_rows = dit_rows - 3
    del seen[:]
    capped = tts.run_batch(batch, shared_cfm=True, continuous_cfm=True)
    _same(out, capped, "capped - uncapped")
    admitted = [s for sl, _, _ in seen for s in sl]
    assert len(seen) >= 2 and len(admitted) == len(slots)
    assert len(set(admitted)) < len(admitted), f"a freed slot is given to a waiting row, got {seen}"


def test_keyword_off_is_the_one_shot_stage():
    """run_batch(shared_cfm=True) without the keyword: the inference_rows calls of the grouped passes, as before -- one per
    (sample_steps, guidance rate) group in first-appearance order, with the group's rows -- and no session"""
    tts, _, (vcfg, vsd, _), _ = build_v3("v3")
    batch = _mix(tts, "v3", vcfg, vsd)
    calls = _spy(tts)
    opened = []
    inner = tts.vits_model.cfm.open_session
    tts.vits_model.cfm.open_session = lambda *a, **k: opened.append(a) or inner(*a, **k)
    tts.run_batch(batch, shared_cfm=True)
    assert opened == []
    # the passes of plan_cfm, one per (sample_steps, guidance rate) group in first-appearance order: (2, 0) request 0 (voice a,
    # 14 prompt frames); (3, 0.7) request 1 (a); (4, 0) request 2 (b: 31 frames cut to T_ref = 20); (2, 0.7) request 4 (c, 17);
    # (3, 0) request 5 (b).  (rows, prompt lengths) per call, as the parent commit issues them for this batch.
    print(f"inference_rows calls: {calls}")
    assert calls == PARENT_CALLS, calls
    with pytest.raises(ValueError):
        tts.run_batch(batch, continuous_cfm=True)
