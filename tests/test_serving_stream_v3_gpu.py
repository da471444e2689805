"""GPU: streaming requests inside the serving sessions on the fp32 small v3 / v4 pipelines of test_pipeline_v3_gpu.py, with the
waveform stage as an open flow-matching session (continuous_cfm=True, cfm_chunk 1 and 2, 4 DiT rows for a mix of a dozen) and as
one-shot shared passes (the keyword off).  The requests are those of test_run_batch_cfm_session_gpu.py: sample_steps 2 / 3 / 4,
one guided request, one LoRA voice; three of them stream (2: two folds; 1: guided; 5: the LoRA voice).

The yardstick of a streaming request is list(tts.run(dict(request, return_fragment=True))) with its voice as the prompt cache:
as many fragments, the same AR tokens, each fragment of the same length and within BAR = 5e-3 of full scale -- the bar
test_serving_cfm_gpu.py holds the server's flow-matching path to, and test_run_batch_cfm_gpu.py the shared stage against run().
A plain request is held to the same bar against run_batch([request])."""
import numpy as np
import pytest

from gsv.serving import Scheduler, plan_online
from test_pipeline_v3_gpu import _build as build_v3
from test_run_batch_cfm_gpu import BAR, _diff
from test_run_batch_cfm_session_gpu import _mix
from test_run_batch_continuous_gpu import _run_batch
from test_serving_gpu import _spy
from test_serving_stream_gpu import _drive, _tokens

pytestmark = pytest.mark.gpu
STREAMS = (1, 2, 5)
PLAIN = (0, 4)
CFM_ROWS = 4


def _run_stream(tts, req):
    """run()'s fragments of the request, its voice being the prompt cache, and the AR tokens [bi][j] it decoded"""
    toks, inner = [], tts._synthesize_batch

    def spy(item, pred, pred_list, *a, **k):
        toks.append([p.cpu().tolist() for p in pred_list])
        return inner(item, pred, pred_list, *a, **k)
    tts._synthesize_batch = spy
    try:
        with tts._with_prompt_cache(dict(req["voice"])):
            frags = list(tts.run(dict({k: v for k, v in req.items() if k != "voice"}, return_fragment=True)))
    finally:
        del tts._synthesize_batch
    return frags, toks


@pytest.fixture(scope="module", params=["v3", "v4"])
def world(request):
    version = request.param
    tts, _, (vcfg, vsd, _), _ = build_v3(version)
    batch = _mix(tts, version, vcfg, vsd)
    alone = {}
    for r in STREAMS:
        alone[r] = _run_stream(tts, batch[r])
        batch[r] = dict(batch[r], **({"streaming_mode": True} if r == 2 else {"return_fragment": True}))
    for r in PLAIN:
        out, preds = _run_batch(tts, [dict(batch[r])])
        alone[r] = (out[0], preds[0])
    assert [len(alone[r][0]) for r in STREAMS] == [1, 2, 1] and all(np.abs(f[1]).max() > 0 for r in STREAMS for f in alone[r][0])
    return version, tts, batch, alone


@pytest.mark.parametrize("cfm_chunk", [1, 2, None], ids=["cfm_chunk1", "cfm_chunk2", "one_shot"])
def test_streaming_through_the_flow_matching_stage(world, cfm_chunk):
    version, tts, batch, alone = world
    kw = {} if cfm_chunk is None else dict(continuous_cfm=True, cfm_rows=CFM_ROWS, cfm_chunk=cfm_chunk)
    order = [2, 0, 1, 4, 5]
    results, plans, frag_steps = {}, {}, {}
    with _spy(tts) as (seen, _), Scheduler(tts, chunk=8, **kw) as sched:
        ticket_of = _drive(sched, batch, [[2, 0], [1], [4, 5]], plans, results, frag_steps)
        stats, slots = sched.stats, sched._pol.slots
        assert sched._ses is None and sched._cfm is None
    assert [ticket_of[r] for r in order] == list(range(5)) and sorted(results) == list(range(5))
    for r in order:
        t = ticket_of[r]
        assert not isinstance(results[t], BaseException), f"request {r} raised {results[t]!r}"
        if r in STREAMS:
            frags, toks = alone[r]
            assert isinstance(results[t], list) and len(results[t]) == len(frags) == len(frag_steps[t])
            assert _tokens(plans[t]) == toks, f"request {r}: other AR tokens than in run()"
            for bi, ((sr, a), (sr0, a0)) in enumerate(zip(results[t], frags)):
                assert sr == sr0 and a.dtype == np.int16 and a.shape == a0.shape, f"request {r} fragment {bi}: {a.shape} vs {a0.shape}"
                d = _diff(a, a0)
                print(f"{version} {cfm_chunk}: request {r} fragment {bi}: {d:.3e} of full scale from run()'s over {a.size} samples")
                assert d <= BAR, f"request {r} fragment {bi}: {d:.3e} of full scale"
        else:
            (sr, audio), tokens = alone[r]
            assert seen[batch[r]["seed"]][0] == tokens
            assert results[t][0] == sr and results[t][1].shape == audio.shape and _diff(results[t][1], audio) <= BAR
    assert stats["exclusive"] == 0 and stats["sessions"] == 1
    assert not any(e[0] == "exclusive" for e in stats["events"]) and [e for e in stats["events"] if e[0] == "close"] == [("close",)]
    idxs = {r: [[int(i) for i in idx] for idx in plans[ticket_of[r]]["idxs"]] if r in STREAMS else seen[batch[r]["seed"]][1] for r in order}
    lengths = [n for r in order for idx in idxs[r] for n in idx]
    cfm_kw = {}
    if cfm_chunk is not None:
        cfm_kw = dict(cfm_folds=[stats["cfm_folds"][t] for t in range(5)], cfm_rows=CFM_ROWS, cfm_chunk=cfm_chunk)
        rows = [row for t in range(5) for f in stats["cfm_folds"][t] for row in f]
        assert len(rows) > CFM_ROWS and {n for n, _ in rows} == {2, 3, 4} and {g for _, g in rows} == {False, True}
        # fold-granular admission: both folds of request 2 went through the session, each fold's rows in chunk order
        adm = [(bi, k) for e in stats["events"] if e[0] == "cfm_admit" for t, bi, k, _ in e[1] if t == ticket_of[2]]
        assert {bi for bi, _ in adm} == {0, 1} and all([k for b, k in adm if b == bi] == sorted(k for b, k in adm if b == bi) for bi in (0, 1))
    plan = plan_online([stats["tickets"][t][0] for t in range(5)], [len(batch[r]["segments"]) for r in order], lengths, slots=slots,
                       chunk=8, streaming={ticket_of[r]: [len(idx) for idx in idxs[r]] for r in STREAMS}, **cfm_kw)
    assert stats["events"] == plan
    assert [e[1:] for e in plan if e[0] == "fragment"].count((ticket_of[2], 0)) == 1 and sum(e[0] == "fragment" for e in plan) == 4
