"""CPU: the AR launch plan of TTS.run_batch -- RNG keys, launch groups and launch size -- for hand-built requests."""
from types import SimpleNamespace

import torch

from gsv.TTS_infer_pack.TTS import TTS


def _stub(max_batch=4, max_seq=256, hz=50, max_sec=0.4):
    return SimpleNamespace(t2s_model=SimpleNamespace(max_batch=max_batch, max_seq=max_seq),
                           configs=SimpleNamespace(hz=hz, max_sec=max_sec))


def _opts(**kw):
    o = TTS._request_options(kw)
    return o


def _plan(lens, batch_size, prompt_phones=3, split_bucket=True):
    segs = [{"phones": list(range(n)), "bert_features": None, "norm_text": "x" * n} for n in lens]
    pd = None if prompt_phones is None else {"phones": [1] * prompt_phones, "bert_features": None}
    data, index = TTS.to_batch(None, segs, prompt_data=pd, batch_size=batch_size, split_bucket=split_bucket)
    return data, index


def test_keys_groups_and_launches():
    d0, _ = _plan([5, 9, 7], batch_size=2)              # to_batch: [[5, 7], [9]] by length
    d1, _ = _plan([4], batch_size=1)
    d2, _ = _plan([6, 8], batch_size=2, prompt_phones=None)
    d3, _ = _plan([5, 6, 7, 8, 9, 10], batch_size=6)
    plans = [
        dict(data=d0, no_prompt=False, P=8, actual_seed=100, opts=_opts(top_k=5, batch_size=2)),
        dict(data=d1, no_prompt=False, P=20, actual_seed=200, opts=_opts(top_k=5)),
        dict(data=d2, no_prompt=True, P=0, actual_seed=300, opts=_opts(top_k=5, batch_size=2)),
        dict(data=d3, no_prompt=False, P=8, actual_seed=400, opts=_opts(top_k=15, batch_size=6)),
    ]
    launches = TTS.plan_batch(_stub(), plans)
    rows = [e for L in launches for e in L]
    # every sentence exactly once
    want = {(r, bi, j) for r, pl in enumerate(plans) for bi, it in enumerate(pl["data"]) for j in range(len(it["all_phones"]))}
    assert sorted((e["r"], e["bi"], e["j"]) for e in rows) == sorted(want)
    # launches hold at most max_batch rows of one group, sorted by length
    for L in launches:
        assert 1 <= len(L) <= 4
        assert len({e["group"] for e in L}) == 1
        assert [e["len"] for e in L] == sorted(e["len"] for e in L)
    key = {(e["r"], e["bi"], e["j"]): e["key"] for e in rows}
    # batched requests: (actual_seed + bi, row in the to_batch batch)
    assert key[(0, 0, 0)] == (100, 0) and key[(0, 0, 1)] == (100, 1) and key[(0, 1, 0)] == (101, 0)
    assert key[(1, 0, 0)] == (200, 0)
    # prompt-free: the naive loop decodes every sentence alone, at row 0
    assert key[(2, 0, 0)] == (300, 0) and key[(2, 0, 1)] == (300, 0)
    # a to_batch batch wider than max_batch is decoded in chunks of max_batch by run(): rows restart at 0
    assert [key[(3, 0, j)] for j in range(6)] == [(400, 0), (400, 1), (400, 2), (400, 3), (400, 0), (400, 1)]
    # groups: requests 0 and 1 share sampling parameters and a launch; top_k 15 and prompt-free decode on their own
    g = {e["r"]: e["group"] for e in rows}
    assert g[0] == g[1] and g[2] != g[0] and g[3] != g[0]
    assert g[2][5] is True and g[0][5] is False
    assert any({e["r"] for e in L} == {0, 1} for L in launches)
    # decode budget as run() gives it: early_stop 20 -> 21 steps unless the K/V arena is shorter
    assert all(e["group"][6] == 21 for e in rows)


def test_arena_bound_budget_separates_groups():
    d0, _ = _plan([30, 80], batch_size=2)
    plans = [dict(data=d0, no_prompt=False, P=100, actual_seed=0, opts=_opts(top_k=5, batch_size=2))]
    launches = TTS.plan_batch(_stub(max_seq=240, max_sec=2), plans)
    rows = [e for L in launches for e in L]
    # run() decodes both sentences in one launch: need = 83 + 100 + 2, so both get 240 - 185 = 55 steps, not 101
    assert {e["group"][6] for e in rows} == {55}
    assert torch.tensor([e["len"] for e in rows]).tolist() == [133, 183]
