"""CPU: the host side of "best_of"  -- the choice among a sentence's candidates, the request key, the
candidate rows of plan_batch, and the two C entries the log-probabilities come through."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from gsv.TTS_infer_pack.TTS import TTS, check_best_of, choose_candidate, select_candidate
from test_run_batch_plan import _opts, _plan, _stub


def _cand(lps, cut=False, n=None):
    """a candidate whose n generated tokens have log-probabilities lps; the finishing step's entry (-9) is not to be counted"""
    n = len(lps) if n is None else n
    return dict(tokens=torch.arange(n), logprobs=np.asarray(list(lps) + [-9.0], dtype=np.float32), n=n, cut=cut)


# ---- select_candidate ----

def test_uncut_beats_cut_whatever_the_scores():
    assert select_candidate([_cand([-0.1, -0.1], cut=True), _cand([-5.0, -7.0])]) == 1
    assert select_candidate([_cand([-5.0, -7.0]), _cand([-0.1, -0.1], cut=True)]) == 0


def test_highest_mean_wins_and_the_finishing_step_is_not_counted():
    cands = [_cand([-2.0, -2.0]), _cand([-1.0, -1.5, -1.0]), _cand([-1.0, -3.0])]
    assert select_candidate(cands) == 1
    # were the finishing entry (-9) counted, the longer candidate would fall behind
    assert select_candidate([_cand([-4.0]), _cand([-4.5, -4.5, -4.5, -4.5])]) == 0
    # the mean, not the sum
    assert select_candidate([_cand([-1.0]), _cand([-0.5] * 10)]) == 1


def test_ties_go_to_the_lowest_index():
    assert select_candidate([_cand([-1.0, -2.0]), _cand([-2.0, -1.0]), _cand([-1.5, -1.5])]) == 0
    assert select_candidate([_cand([-3.0]), _cand([-1.0, -2.0]), _cand([-2.0, -1.0])]) == 1


def test_all_cut_highest_mean_wins():
    assert select_candidate([_cand([-2.0], cut=True), _cand([-1.0], cut=True), _cand([-1.5], cut=True)]) == 1


def test_an_empty_candidate_loses():
    assert select_candidate([_cand([], n=0), _cand([-30.0])]) == 1
    assert select_candidate([_cand([], n=0), _cand([], n=0)]) == 0
    # ... but not against a cut one
    assert select_candidate([_cand([-1.0], cut=True), _cand([], n=0)]) == 1


def test_the_mean_is_taken_in_float64_and_torch_tensors_are_read_too():
    a = _cand([-1.0, -1.0 - 2.0 ** -23])
    b = dict(a, logprobs=torch.tensor([-1.0 - 2.0 ** -23, -1.0, -9.0]))
    _, rec = choose_candidate({}, [a, b])
    assert rec[0]["mean_logprob"] == rec[1]["mean_logprob"] == -1.0 - 2.0 ** -24
    assert [r["chosen"] for r in rec] == [True, False]


def test_a_callable_overrides_the_default():
    cands = [_cand([-1.0]), _cand([-2.0]), _cand([-3.0], cut=True)]
    seen = []
    k, rec = choose_candidate({"best_of_score": lambda c: seen.append(c) or 2}, cands)
    assert k == 2 and seen == [cands]
    assert rec == [dict(n=1, mean_logprob=-1.0, cut=False, chosen=False), dict(n=1, mean_logprob=-2.0, cut=False, chosen=False),
                   dict(n=1, mean_logprob=-3.0, cut=True, chosen=True)]
    assert choose_candidate({}, cands)[0] == 0
    for bad in (3, -1, 1.0, None, True):
        with pytest.raises(ValueError):
            choose_candidate({"best_of_score": lambda c: bad}, cands)


# ---- the request key ----

def _resolver(version="v2"):
    return SimpleNamespace(configs=SimpleNamespace(version=version, use_vocoder=version in ("v3", "v4")),
                           _request_options=TTS._request_options)


def test_absent_or_one_leaves_the_options_as_they_are():
    plain = TTS._request_options({"top_k": 7})
    assert "best_of" not in plain and "best_of_score" not in plain
    assert TTS._request_options({"top_k": 7, "best_of": 1}) == plain
    assert TTS._request_options({"top_k": 7, "best_of": None}) == plain
    assert TTS._request_options({"top_k": 7, "best_of": 1, "best_of_score": len}) == plain
    assert TTS._resolve_options(_resolver(), {"top_k": 7, "best_of": 1}) == TTS._resolve_options(_resolver(), {"top_k": 7})
    o = TTS._resolve_options(_resolver(), {"top_k": 7, "best_of": 3, "best_of_score": len})
    assert o["best_of"] == 3 and o["best_of_score"] is len
    assert {k: v for k, v in o.items() if not k.startswith("best_of")} == TTS._resolve_options(_resolver(), {"top_k": 7})
    assert TTS._resolve_options(_resolver(), {"best_of": 16})["best_of"] == 16


@pytest.mark.parametrize("bad", [0, 17, 2.5, "3", -2, True, [2]])
def test_other_values_are_refused_before_any_gpu_work(bad):
    with pytest.raises(ValueError, match="best_of"):
        TTS._resolve_options(_resolver(), {"best_of": bad})


def test_the_naive_and_prompt_free_loops_are_refused():
    with pytest.raises(ValueError, match="parallel_infer"):
        TTS._resolve_options(_resolver(), {"best_of": 2, "parallel_infer": False})
    assert TTS._resolve_options(_resolver(), {"best_of": 1, "parallel_infer": False})["parallel_infer"] is False
    o = TTS._resolve_options(_resolver(), {"best_of": 2})
    check_best_of(o, no_prompt=False)
    with pytest.raises(ValueError, match="prompt"):
        check_best_of(o, no_prompt=True)
    check_best_of(TTS._request_options({}), no_prompt=True)
    with pytest.raises(ValueError, match="callable"):
        TTS._resolve_options(_resolver(), {"best_of": 2, "best_of_score": "mean"})


# ---- plan_batch ----

def _plans(best_of):
    d0, _ = _plan([5, 9, 7], batch_size=2)              # to_batch: [[5, 7], [9]] by length
    d1, _ = _plan([4, 6], batch_size=2)
    extra = {} if best_of is None else {"best_of": best_of}
    return [dict(data=d0, no_prompt=False, P=8, actual_seed=100, opts=_opts(top_k=5, batch_size=2, **extra)),
            dict(data=d1, no_prompt=False, P=20, actual_seed=200, opts=_opts(top_k=5, batch_size=2))]


@pytest.mark.parametrize("mixed", [False, True])
def test_candidate_rows_keys_and_launch_size(mixed):
    launches = TTS.plan_batch(_stub(), _plans(3), mixed_sampling=mixed)
    plain = TTS.plan_batch(_stub(), _plans(None), mixed_sampling=mixed)
    rows = [e for L in launches for e in L]
    base = {(e["r"], e["bi"], e["j"]): e for L in plain for e in L}
    # three entries per sentence of request 0, candidate c with the key (seed, row + 1024 c); candidate 0 has the plain key
    for (r, bi, j), e0 in base.items():
        mine = sorted((e for e in rows if (e["r"], e["bi"], e["j"]) == (r, bi, j)), key=lambda e: e.get("cand", 0))
        if r == 1:
            assert mine == [e0], "the request without the key has the entries it has without its neighbour's key"
            continue
        assert [e["cand"] for e in mine] == [0, 1, 2]
        assert [e["key"] for e in mine] == [(e0["key"][0], e0["key"][1] + 1024 * c) for c in range(3)]
        assert mine[0]["key"] == e0["key"]
        for e in mine:
            assert {k: v for k, v in e.items() if k not in ("cand", "key")} == {k: v for k, v in e0.items() if k != "key"}
    assert len(rows) == 3 * 3 + 2
    for L in launches:
        assert 1 <= len(L) <= 4 and len({e["group"] for e in L}) == 1
    # best_of = 1 plans what no key plans
    assert TTS.plan_batch(_stub(), _plans(1), mixed_sampling=mixed) == plain
    assert 1024 * 15 + 63 < 2 ** 24, "the hash gives the row 24 bits"


# ---- ABI ----

def test_the_header_declares_and_the_library_exports_the_two_entries():
    from gsv import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "gsv.h")).read()
    assert re.search(r"int gsv_t2s_set_logprobs\(gsv_t2s_t\* h, float\* out_logp\);", hdr)
    assert re.search(r"int gsv_op_token_logprob\(const float\* logits, int B, int vocab, int vocab_eff, const int32_t\* tokens, "
                     r"float\* out,\s+gsv_stream_t stream\);", hdr)
    assert os.path.exists(build.build(verbose=False))
    l = _lib.lib()
    assert hasattr(l, "gsv_t2s_set_logprobs") and hasattr(l, "gsv_op_token_logprob")
    assert {"gsv_t2s_set_logprobs", "gsv_op_token_logprob"} <= set(_lib.EXPORTS)
    assert l.gsv_abi_version() == 1
