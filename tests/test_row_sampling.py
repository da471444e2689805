"""CPU: per-row sampling parameters -- the AR launch plan of TTS.run_batch(mixed_sampling=True) and the argument check of
Text2SemanticDecoder._run(row_sampling=...)."""
from types import SimpleNamespace

import pytest
import torch

from gsv.TTS_infer_pack.TTS import TTS
from test_run_batch_plan import _opts, _plan, _stub


def _plans():
    """the requests of test_run_batch_plan.test_keys_groups_and_launches"""
    d0, _ = _plan([5, 9, 7], batch_size=2)
    d1, _ = _plan([4], batch_size=1)
    d2, _ = _plan([6, 8], batch_size=2, prompt_phones=None)
    d3, _ = _plan([5, 6, 7, 8, 9, 10], batch_size=6)
    return [
        dict(data=d0, no_prompt=False, P=8, actual_seed=100, opts=_opts(top_k=5, batch_size=2)),
        dict(data=d1, no_prompt=False, P=20, actual_seed=200, opts=_opts(top_k=5)),
        dict(data=d2, no_prompt=True, P=0, actual_seed=300, opts=_opts(top_k=5, batch_size=2)),
        dict(data=d3, no_prompt=False, P=8, actual_seed=400, opts=_opts(top_k=15, batch_size=6)),
    ]


def _sentences(plans):
    return sorted((r, bi, j) for r, pl in enumerate(plans) for bi, it in enumerate(pl["data"]) for j in range(len(it["all_phones"])))


def test_mixed_sampling_merges_groups_and_keeps_rows_keys_and_budget():
    plans = _plans()
    mb = 4
    launches = TTS.plan_batch(_stub(max_batch=mb), plans, mixed_sampling=True)
    rows = [e for L in launches for e in L]
    assert sorted((e["r"], e["bi"], e["j"]) for e in rows) == _sentences(plans)          # every sentence exactly once
    # the tuple keeps its seven slots: the sampling slots are None, slots 4-6 still say what they said
    for e in rows:
        assert len(e["group"]) == 7 and e["group"][:4] == (None,) * 4
        assert e["group"][4] is True and e["group"][5] is (e["r"] == 2) and e["group"][6] == 21
    g = {e["r"]: e["group"] for e in rows}
    assert g[0] == g[1] == g[3] and g[2] != g[0]                                        # top_k 5, 5 and 15 share; prompt-free apart
    for L in launches:
        assert 1 <= len(L) <= mb and len({e["group"] for e in L}) == 1
        assert [e["len"] for e in L] == sorted(e["len"] for e in L)
    # requests 0, 1 and 3 hold 3 + 1 + 6 = 10 sentences: launches of 4, 4 and 2 rows filled together, sorted by length
    shared = [L for L in launches if L[0]["group"] == g[0]]
    assert [len(L) for L in shared] == [4, 4, 2]
    assert any(len({e["sampling"][0] for e in L}) == 2 for L in shared), "no launch mixes top_k 5 with top_k 15"
    assert [len(L) for L in launches if L[0]["group"] == g[2]] == [2]
    # each row carries its request's options
    for e in rows:
        o = plans[e["r"]]["opts"]
        assert e["sampling"] == (o["top_k"], o["top_p"], o["temperature"], o["repetition_penalty"])
    # RNG keys are those of the default plan
    default = TTS.plan_batch(_stub(max_batch=mb), plans)
    key = {(e["r"], e["bi"], e["j"]): e["key"] for L in default for e in L}
    assert {(e["r"], e["bi"], e["j"]): e["key"] for e in rows} == key
    # with room for all ten rows the three requests are one launch where the default plan needs two
    wide = TTS.plan_batch(_stub(max_batch=16), plans, mixed_sampling=True)
    assert sorted(len(L) for L in wide) == [2, 10]
    assert sorted(len(L) for L in TTS.plan_batch(_stub(max_batch=16), plans)) == [2, 4, 6]


def test_default_plan_is_unchanged_by_the_keyword():
    plans = _plans()
    a = TTS.plan_batch(_stub(), plans)
    b = TTS.plan_batch(_stub(), plans, mixed_sampling=False)
    assert a == b
    assert all("sampling" not in e and None not in e["group"] for L in a for e in L)


def test_ar_stage_hands_rows_over_only_when_a_launch_mixes_them():
    """_ar_stage with a recording decoder: row_sampling goes to the launches whose rows differ, never without the keyword"""
    calls = []

    def _run(x, prompts, bert, top_k, top_p, early_stop, temperature, repetition_penalty, **kw):
        calls.append((top_k, top_p, temperature, repetition_penalty, kw.get("row_sampling"), len(x)))
        return [torch.zeros(3, dtype=torch.long)] * len(x), [1] * len(x)

    stub = _stub(max_batch=4)
    stub.t2s_model._run = _run
    stub.plan_batch = lambda plans, **kw: TTS.plan_batch(stub, plans, **kw)
    stub._kept_tokens = lambda p, i, no_prompt: (p, i)
    stub._wait_stream = lambda: None
    voice = dict(prompt_semantic=torch.zeros(1, 8, dtype=torch.long))
    for mixed in (False, True):
        plans = _plans()
        for pl in plans:
            pl["voice"] = voice
        calls.clear()
        TTS._ar_stage(stub, plans, mixed_sampling=mixed)
        assert sum(c[5] for c in calls) == 12
        if not mixed:
            assert all(c[4] is None for c in calls)
            continue
        for c in calls:
            if c[4] is None:
                continue
            assert len(c[4]) == c[5] and len(set(c[4])) > 1
            assert {s[0] for s in c[4]} == {5, 15}
        assert any(c[4] is not None for c in calls) and any(c[4] is None for c in calls)   # the prompt-free launch is uniform


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the argument check")


def test_run_refuses_a_row_sampling_length_mismatch_before_any_library_call(monkeypatch):
    from gsv import _lib
    from gsv.AR.models.t2s_model import Text2SemanticDecoder
    monkeypatch.setattr(_lib, "lib", lambda: _NoLibrary())
    model = SimpleNamespace(_loaded=True, device="cpu", max_seq=256, vocab_size=1025, _h=None)
    x = [torch.zeros(5, dtype=torch.long)] * 3
    with pytest.raises(ValueError, match="2 sampling tuples for 3 rows"):
        Text2SemanticDecoder._run(model, x, torch.zeros(3, 4, dtype=torch.long), [None] * 3, 5, 1.0, 20, 1.0, 1.35,
                                  eos_mask_steps=1, row_sampling=[(5, 1.0, 1.0, 1.35)] * 2)
    with pytest.raises(ValueError, match="4 sampling tuples for 3 rows"):
        Text2SemanticDecoder.infer_panel_batch_infer(model, x, None, torch.zeros(3, 4, dtype=torch.long), [None] * 3,
                                                     row_sampling=[(5, 1.0, 1.0, 1.35)] * 4)


def test_ctypes_row_struct_is_sixteen_bytes():
    import ctypes as C
    from gsv import _lib
    assert C.sizeof(_lib.RowSampling) == 16
    assert [n for n, _ in _lib.RowSampling._fields_] == ["top_k", "top_p", "temperature", "repetition_penalty"]
