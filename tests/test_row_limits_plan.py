"""CPU: per-row limits in the plans -- TTS.plan_batch(mixed_limits=True), the rows Scheduler(mixed_limits=True) brings for the
requests that used to be exclusive, the limit tuples Text2SemanticDecoder hands to the engine, and the ABI."""
import os
import re


from conftest import ROOT
from gsv.TTS_infer_pack.TTS import BEST_OF_ROW_STRIDE, TTS
from test_run_batch_plan import _opts, _plan, _stub


def _plans():
    """a plain, a naive, a prompt-free and an arena-short request (max_seq 240: 160 + 40 + 2 leaves 38 of 41 steps)"""
    d0, _ = _plan([5, 9], batch_size=2)
    d1, _ = _plan([6, 7], batch_size=2)
    d2, _ = _plan([6, 8], batch_size=2, prompt_phones=None)
    d3, _ = _plan([160], batch_size=1)
    return [
        dict(data=d0, no_prompt=False, P=8, actual_seed=100, opts=_opts(top_k=5, batch_size=2)),
        dict(data=d1, no_prompt=False, P=8, actual_seed=200, opts=_opts(top_k=5, batch_size=2, parallel_infer=False)),
        dict(data=d2, no_prompt=True, P=0, actual_seed=300, opts=_opts(top_k=5, batch_size=2)),
        dict(data=d3, no_prompt=False, P=40, actual_seed=400, opts=_opts(top_k=5)),
    ]


def _tts(max_batch=16):
    return _stub(max_batch=max_batch, max_seq=240, max_sec=0.8)     # early stop 40: 41 steps wanted


def test_mixed_limits_puts_the_four_kinds_into_one_launch():
    plans = _plans()
    launches = TTS.plan_batch(_tts(), plans, mixed_sampling=True, mixed_limits=True)
    assert [len(L) for L in launches] == [7]
    rows = {(e["r"], e["bi"], e["j"]): e for e in launches[0]}
    assert [e["len"] for e in launches[0]] == sorted(e["len"] for e in launches[0])
    for e in rows.values():
        assert e["group"] == (None,) * 7
    # the sentence lengths include the 3 prompt phones of _plan
    assert {k: (e["limits"], e["no_prompt"]) for k, e in rows.items()} == {
        (0, 0, 0): ((1, 40, 41), False), (0, 0, 1): ((1, 40, 41), False),
        (1, 0, 0): ((11, 40, 41), False), (1, 0, 1): ((11, 40, 41), False),
        (2, 0, 0): ((11, 40, 41), True), (2, 0, 1): ((11, 40, 41), True),
        (3, 0, 0): ((1, 40, 240 - (163 + 40 + 2)), False),
    }
    # the keys are the default plan's: batched rows (seed + bi, j), naive and prompt-free rows row 0
    assert {k: e["key"] for k, e in rows.items()} == {
        (0, 0, 0): (100, 0), (0, 0, 1): (100, 1), (1, 0, 0): (200, 0), (1, 0, 1): (200, 0), (2, 0, 0): (300, 0), (2, 0, 1): (300, 0),
        (3, 0, 0): (400, 0)}
    default = TTS.plan_batch(_tts(), plans)
    assert {(e["r"], e["bi"], e["j"]): e["key"] for L in default for e in L} == {k: e["key"] for k, e in rows.items()}
    # mixed_limits alone keeps the sampling groups
    only = TTS.plan_batch(_tts(), plans, mixed_limits=True)
    assert all(e["group"][:4] == (5, 1, 1, 1.35) and e["group"][4:] == (None,) * 3 and "sampling" not in e for L in only for e in L)
    # max_batch still cuts the launches
    assert [len(L) for L in TTS.plan_batch(_tts(max_batch=4), plans, mixed_sampling=True, mixed_limits=True)] == [4, 3]


def test_without_the_keyword_the_launches_are_the_documented_groups():
    plans = _plans()
    got = TTS.plan_batch(_tts(), plans)
    assert got == TTS.plan_batch(_tts(), plans, mixed_limits=False)
    # by hand, from the grouping rule: one group per (sampling, parallel_infer, prompt-free, budget) in order of first
    # appearance, rows sorted by length (text + 3 prompt phones + P)
    s = (5, 1, 1, 1.35)

    def row(r, j, n, P, key, g):
        return dict(r=r, bi=0, j=j, len=n + 3 * (P > 0) + P, group=s + g, key=key)
    want = [
        [row(0, 0, 5, 8, (100, 0), (True, False, 41)), row(0, 1, 9, 8, (100, 1), (True, False, 41))],
        [row(1, 0, 6, 8, (200, 0), (False, False, 41)), row(1, 1, 7, 8, (200, 0), (False, False, 41))],
        [row(2, 0, 6, 0, (300, 0), (True, True, 41)), row(2, 1, 8, 0, (300, 0), (True, True, 41))],
        [row(3, 0, 160, 40, (400, 0), (True, False, 35))],
    ]
    assert got == want


def test_best_of_candidates_keep_their_keys_under_mixed_limits():
    d, _ = _plan([5, 9], batch_size=2)
    plans = [dict(data=d, no_prompt=False, P=8, actual_seed=7, opts=_opts(top_k=5, batch_size=2, best_of=3))]
    rows = [e for L in TTS.plan_batch(_tts(), plans, mixed_sampling=True, mixed_limits=True) for e in L]
    assert sorted((e["j"], e["cand"], e["key"]) for e in rows) == \
        [(j, c, (7, j + BEST_OF_ROW_STRIDE * c)) for j in range(2) for c in range(3)]
    assert all(e["limits"] == (1, 40, 41) and e["no_prompt"] is False for e in rows)


def _scheduler(**kw):
    from gsv.serving import Scheduler
    tts = _tts()
    tts.vits_model = object()
    tts.plan_batch = lambda plans, **k: TTS.plan_batch(tts, plans, **k)
    return Scheduler(tts, slots=8, **kw)


def test_scheduler_session_rows_for_the_four_kinds():
    plans = _plans()
    d, _ = _plan([5, 9], batch_size=2)
    best = dict(data=d, no_prompt=False, P=8, actual_seed=7, opts=_opts(top_k=5, batch_size=2, best_of=3))
    d, _ = _plan([195], batch_size=1)
    full = dict(data=d, no_prompt=False, P=40, actual_seed=9, opts=_opts(top_k=5))      # 198 + 40 + 2 = 240: no room at all
    old, new = _scheduler(), _scheduler(mixed_limits=True)
    assert old._session_rows(plans[0]) is not None
    assert [old._session_rows(pl) for pl in plans[1:] + [best, full]] == [None] * 5
    for pl, lim, free in zip(plans, [(1, 40, 41), (11, 40, 41), (11, 40, 41), (1, 40, 35)], [False, False, True, False]):
        rows = new._session_rows(pl)
        assert [(e["bi"], e["j"]) for e in rows] == [(0, j) for j in range(len(pl["data"][0]["all_phones"]))]
        assert all(e["limits"] == lim and e["no_prompt"] is free and "sampling" in e for e in rows)
    rows = new._session_rows(best)
    assert [(e["j"], e["cand"]) for e in rows] == [(j, c) for j in range(2) for c in range(3)]
    assert [e["key"] for e in rows] == [(7, j + BEST_OF_ROW_STRIDE * c) for j in range(2) for c in range(3)]
    assert new._session_rows(full) is None
    assert new.stats["exclusive"] == 0 and "mixed_limits" not in old.stats


def test_a_streaming_best_of_request_brings_its_candidate_rows_fold_by_fold():
    """a fold of a streaming request counts candidate rows: two folds of 2 and 1 sentences, best_of=3 -> 6 and 3 rows"""
    d, _ = _plan([5, 9, 7], batch_size=2, split_bucket=False)
    assert [len(it["all_phones"]) for it in d] == [2, 1]
    pl = dict(data=d, no_prompt=False, P=8, actual_seed=7, frags=[None, None],
              opts=_opts(top_k=5, batch_size=2, best_of=3, return_fragment=True, split_bucket=False))
    for kw, rows, folds in ((dict(mixed_limits=True), 9, [6, 3]), ({}, 0, None)):
        sched = _scheduler(shared_hubert=False, shared_bert=False, **kw)
        sched.tts._plan_request = lambda req, **k: dict(pl)
        t = sched.submit(dict(return_fragment=True))
        out = []
        sched._intake(out)                                          # must not raise: it runs outside any per-request try
        assert out == []
        if folds is None:                                           # without the keyword the request is exclusive, as before
            assert list(sched._pol.fifo) == [[t, 0, 0, True]] and not sched._pol.stream
            continue
        assert list(sched._pol.fifo) == [[t, rows, 0, False]]
        st = sched._pol.stream[t]
        assert st.missing == dict(enumerate(folds)) and st.fold == [0] * 6 + [1] * 3
        assert [(e["bi"], e["j"], e["cand"]) for e in sched._rows[t]] == \
            [(0, j, c) for j in range(2) for c in range(3)] + [(1, 0, c) for c in range(3)]


def test_row_limit_tuples_bound_the_budget_by_the_arena():
    from gsv.AR.models.t2s_model import row_limit_tuples
    lims, budgets, short = row_limit_tuples([(1, 40, 41), (11, None, 30), (1, 40, 41), (3, 5, 41)], [50, 50, 210, 238], 240)
    assert lims == [(1, 40, 41), (11, -1, 30), (1, -1, 30), (3, -1, 2)] and budgets == [41, 30, 30, 2] and short
    assert row_limit_tuples([(1, 40, 41)], [50], 240) == ([(1, 40, 41)], [41], False)
    assert row_limit_tuples([(1, 40, 41)], [240], 240)[1] == [0]


def test_the_header_declares_and_the_library_binds_row_limits():
    import ctypes as C
    from gsv import _lib, build
    src = open(os.path.join(ROOT, "include", "gsv.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"typedef\s+struct\s*\{\s*int\s+eos_mask_steps\s*;\s*int\s+early_stop_num\s*;\s*int\s+max_steps\s*;\s*int\s+reserved\s*;"
                     r"\s*\}\s*gsv_row_limits_t\s*;", src)
    assert re.search(r"\bint\s+gsv_t2s_set_row_limits\s*\(\s*gsv_t2s_t\s*\*\s*h\s*,\s*const\s+gsv_row_limits_t\s*\*\s*rows\s*,\s*int\s+B\s*\)\s*;",
                     src)
    assert C.sizeof(_lib.RowLimits) == 16 and [f[0] for f in _lib.RowLimits._fields_] == \
        ["eos_mask_steps", "early_stop_num", "max_steps", "reserved"]
    assert "gsv_t2s_set_row_limits" in _lib.EXPORTS
    build.build(verbose=False)
    l = _lib.lib()
    assert hasattr(l, "gsv_t2s_set_row_limits") and len(l.gsv_t2s_set_row_limits.argtypes) == 3
    assert l.gsv_abi_version() == 1
