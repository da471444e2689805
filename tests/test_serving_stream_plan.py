"""CPU: streaming requests in gsv.serving.plan_online -- the schedule of a Scheduler that delivers a `return_fragment` request
fold by fold from inside its sessions -- as properties over seeded random traces, with and without the flow-matching session;
and the scheduler's own intake decision (which streaming requests stay exclusive) over a pipeline stub that does no GPU work."""
import types

import pytest

from gsv.serving import Scheduler, plan_online
from _serving_cases import stream_case as _case

CASES = 200


@pytest.mark.parametrize("cfm", [False, True], ids=["sovits", "cfm"])
@pytest.mark.parametrize("seed", range(CASES))
def test_fragments_in_order_never_early_and_no_barrier(seed, cfm):
    c, streaming, folds = _case(seed, cfm)
    trace = plan_online(**c, streaming=streaming, with_steps=True)
    assert [e for _, e in trace] == plan_online(**c, streaming=streaming)
    live = {r: f for r, f in streaming.items() if r not in c["exclusive"]}
    fold_of = {r: [bi for bi, k in enumerate(f) for _ in range(k)] for r, f in live.items()}
    back_at = {}                                    # (r, bi) -> the step its last row finished in
    left = {(r, bi): k for r, f in live.items() for bi, k in enumerate(f)}
    emitted = {r: [] for r in live}
    audio_at = {}                                   # (r, bi) -> the step of the pass that made its audio
    for step, e in trace:
        if e[0] == "advance":
            for r, row in e[2]:
                if r in live:
                    left[(r, fold_of[r][row])] -= 1
                    if left[(r, fold_of[r][row])] == 0:
                        back_at[(r, fold_of[r][row])] = step
        elif e[0] == "wave":
            assert not set(e[1]) & set(live), "a streaming request is never waved as a whole"
            for f in (e[2] if len(e) > 2 else []):
                assert back_at[f] == step, "a ready fold goes into the pass of the step it became ready in"
                audio_at[f] = step
        elif e[0] == "vocode":
            audio_at.update({f: step for f in e[1] if f[0] in live})
        elif e[0] == "cfm_admit":
            for r, bi, _, _ in e[1]:
                assert r not in live or back_at[(r, bi)] <= step, "a fold's rows are admitted once its sentences are back"
        elif e[0] == "deliver":
            assert not set(e[1]) & set(live)
        elif e[0] == "fragment":
            _, r, bi = e
            assert bi == len(emitted[r]), "fragments come in fold order"
            assert back_at[(r, bi)] <= step, "a fragment never comes before the step its last row finished in"
            if not cfm or c["cfm_folds"][r][bi]:
                assert audio_at[(r, bi)] <= step
            emitted[r].append(step)
        elif e[0] == "exclusive":
            assert e[1] in c["exclusive"], "a streaming request is no barrier"
    assert {r: len(s) for r, s in emitted.items()} == {r: len(f) for r, f in live.items()}, "every fold is emitted exactly once"
    assert sorted(e[1] for _, e in trace if e[0] == "exclusive") == sorted(c["exclusive"])
    if not cfm:
        # the first fragment does not wait for the last sentence: it is out in the step its own fold came back
        for r in live:
            assert emitted[r][0] == back_at[(r, 0)]
    # the schedule of the rows does not depend on who streams: admissions and advances are those of the plain trace
    plain = plan_online(**c)
    # (with a flow-matching session an exclusive request also waits for that session, whose timing streaming does change)
    assert (cfm and c["exclusive"]) or [e for e in plan_online(**c, streaming=streaming) if e[0] in ("admit", "advance")] == [e for e in plain if e[0] in ("admit", "advance")]
    if not live:
        assert [e for _, e in trace] == plain


@pytest.mark.parametrize("seed", range(60))
def test_without_streaming_requests_the_trace_is_the_parents(seed):
    for cfm in (False, True):
        c, _, _ = _case(seed, cfm)
        assert plan_online(**c, streaming={}) == plan_online(**c, streaming=None) == plan_online(**c)
        # naming only exclusive requests changes nothing either: their entry is not read
        assert plan_online(**c, streaming={r: [99] for r in c["exclusive"]}) == plan_online(**c)


def test_no_close_and_no_exclusive_on_account_of_a_streaming_request():
    # three requests in one burst, the middle one streams: one session, one close at the very end
    args = dict(arrivals=[0, 0, 1], rows_per_request=[2, 3, 2], lengths=[5, 9, 3, 20, 4, 7, 7], slots=4, chunk=8)
    trace = plan_online(**args, streaming={1: [2, 1]})
    assert not any(e[0] == "exclusive" for e in trace) and [e for e in trace if e[0] == "close"] == [("close",)] and trace[-1] == ("close",)
    assert [e for e in trace if e[0] == "fragment"] == [("fragment", 1, 0), ("fragment", 1, 1)]
    # fold 1 (one row of 4 steps) is back a step before fold 0 (a row of 20): its pass runs at once, its fragment waits
    assert ("wave", [0], [(1, 1)]) in trace and trace.index(("wave", [0], [(1, 1)])) < trace.index(("fragment", 1, 0))
    # the parent's schedule for the same request, exclusive: a close in front of it and the barrier itself
    parent = plan_online(arrivals=[0, 0, 1], rows_per_request=[2, 0, 2], lengths=[5, 9, 7, 7], slots=4, chunk=8, exclusive=[1])
    assert ("exclusive", 1) in parent and parent.count(("close",)) == 2
    with pytest.raises(ValueError):
        plan_online(**args, streaming={1: [2, 2]})


# ---- the scheduler's intake: which streaming requests stay exclusive

class _Pipe:
    """what Scheduler._intake touches, without a GPU: plans are handed in ready-made"""
    from gsv.TTS_infer_pack.TTS import TTS as _T
    plan_batch = _T.plan_batch

    def __init__(self):
        self.configs = types.SimpleNamespace(use_vocoder=False, hz=50, max_sec=2)         # early stop at 100 tokens
        self.t2s_model = types.SimpleNamespace(max_batch=4, max_seq=256)
        self.vits_model = object()
        self.asked = []

    def _plan_request(self, req, **kw):
        import torch
        self.asked.append((req["name"], kw))
        if req.get("return_fragment") and not kw.get("fragments"):
            raise ValueError("run_batch returns whole utterances")
        opts = dict(top_k=5, top_p=1, temperature=1, repetition_penalty=1.35, parallel_infer=req.get("parallel_infer", True),
                    return_fragment=bool(req.get("return_fragment")))
        if "best_of" in req:
            opts["best_of"] = req["best_of"]
        data = [dict(all_phones=[torch.zeros(n, dtype=torch.long) for n in fold]) for fold in req["folds"]]
        return dict(opts=opts, no_prompt=bool(req.get("no_prompt")), P=20, actual_seed=1, data=data, frags=[None] * len(data))


def test_a_streaming_request_is_exclusive_only_for_the_reasons_a_plain_one_is():
    pipe = _Pipe()
    sched = Scheduler(pipe, slots=4, chunk=8, shared_hubert=False, shared_bert=False)
    reqs = [dict(name="stream", folds=[[10, 12], [9]], streaming_mode=True),
            dict(name="plain", folds=[[10, 12], [9]]),
            dict(name="stream-free", folds=[[10]], return_fragment=True, no_prompt=True),
            dict(name="stream-best", folds=[[10]], return_fragment=True, best_of=3),
            dict(name="stream-naive", folds=[[10]], return_fragment=True, parallel_infer=False),
            dict(name="stream-cut", folds=[[10, 140]], return_fragment=True),                # 140 + 20 + 2 + 101 > 256
            dict(name="plain-cut", folds=[[10, 140]])]
    tickets = [sched.submit(r) for r in reqs]
    out = []
    sched._intake(out)
    assert out == []
    assert [(n, kw) for n, kw in pipe.asked] == [(r["name"], {"fragments": True} if "stream" in r["name"] else {}) for r in reqs], \
        "the planner's keyword is passed for streaming requests only"
    pol = sched._pol
    assert [(e[0], e[1], e[3]) for e in pol.fifo] == [(0, 3, False), (1, 3, False), (2, 0, True), (3, 0, True), (4, 0, True),
                                                     (5, 0, True), (6, 0, True)]
    assert list(pol.stream) == [tickets[0]] and pol.stream[0]["fold"] == [0, 0, 1] and pol.stream[0]["n"] == 2
    assert [(e["bi"], e["j"]) for e in sched._rows[0]] == [(0, 0), (0, 1), (1, 0)], "rows are admitted in (bi, j) order"
    assert sched._requests[2]["return_fragment"] is True and sched._requests[0]["opts"]["return_fragment"] is True
