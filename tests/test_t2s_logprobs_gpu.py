"""GPU: the taken token's log-probability of every decode step (gsv_t2s_set_logprobs) on both decode
paths: sample_step_kernel (fp32 launch path, and step 0 of every decode) and the persistent engine's LOGP kernels (fp16).

* parity: with dump_logits=True every executed step of every row -- step 0 and the finishing step included -- equals the fp64
  mirror of _logprob_ref.py on the dumped logits and the taken token, under the bar derived there; entries after a row's last
  step keep the fill;
* forcing: under force_tokens the entries are the forced tokens' (rows forced to EOS at different steps; a forced EOS at the
  masked step 0 gives -inf);
* sampling is untouched: tokens and idx with and without log-probabilities are equal, with scalar sampling, row_sampling and
  rng_keys;
* the hook holds for one decode; sessions give every row the one-shot decode's values bit for bit, whatever the chunk, and an
  admission leaves its neighbours' entries alone.
"""
import numpy as np
import pytest
import torch

from _logprob_ref import check_row
from test_t2s_ragged_gpu import DEV, _dev, _engine, _rows

pytestmark = pytest.mark.gpu
FOUR = [(1, 1.0, 1.0, 1.35), (15, 1.0, 1.0, 1.35), (5, 0.8, 0.9, 1.0), (0, 0.6, 1.2, 1.2)]


@pytest.fixture(scope="module")
def small():
    from oracle import cases
    cfg, sd, *_ = cases.t2s_case_inputs(cases.T2S_CASES["t2s_small_greedy"])
    return cfg, _engine(cfg, sd, torch.float32, max_batch=64, max_seq=320)


@pytest.fixture(scope="module")
def v2():
    from gsv import synthetic as S
    cfg = S.T2S_V2_CONFIG
    sd = S.make_t2s_state_dict(cfg, seed=0, suppress_eos=True)
    return cfg, _engine(cfg, sd, torch.float16, max_batch=64, max_seq=320)


def _inputs(cfg, B, seed):
    xs, berts, prompts = _rows(cfg, B, seed=seed, zh_bert=True)
    xd, bd = _dev(xs, berts)
    return xd, bd, [p.to(DEV) for p in prompts]


def _check_against_mirror(eng, V, idx, taken, what):
    """every executed step of every row against the mirror; taken[b][s] = the token row b took at step s.  Returns the largest
    |error| / bar."""
    L = eng.last_logits_dump.cpu().numpy()
    buf = eng.last_logprob_buffer.cpu().numpy()
    worst = 0.0
    for b, n in enumerate(idx):
        lp = eng.last_logprobs[b].cpu().numpy()
        assert lp.shape == (n + 1,) and lp.dtype == np.float32
        for s in range(n + 1):
            worst = max(worst, check_row(lp[s], L[s, b], V - 1 if s < 1 else V, taken[b][s], f"{what} row {b} step {s}"))
        assert np.isnan(buf[b, n + 1:]).all(), f"{what} row {b}: entries after step {n} lost the fill"
    print(f"[logprobs] {what}: {sum(n + 1 for n in idx)} (row, step) entries, largest |error| / bar = {worst:.3f}")
    return worst


def _taken_sampled(eng, B, idx):
    drawn = eng.last_drawn_dump.cpu().numpy()
    return [[int(drawn[s, b, 0]) for s in range(idx[b] + 1)] for b in range(B)]


def test_fp32_launch_path_every_step_matches_the_mirror(small):
    cfg, eng = small
    B, V = 5, cfg["model"]["vocab_size"]
    xd, bd, pd = _inputs(cfg, B, seed=23)
    assert len({p.numel() for p in pd}) > 1
    kw = dict(top_k=15, top_p=1.0, temperature=1.0, early_stop_num=24, repetition_penalty=1.35, seed=77)
    ys, idx = eng.infer_panel_batch_infer(xd, None, pd, bd, dump_logits=True, logprobs=True, **kw)
    assert eng.decode_info()[0] == 0
    taken = _taken_sampled(eng, B, idx)
    for b in range(B):
        assert taken[b][:idx[b]] == ys[b].tolist()[pd[b].numel():]
    _check_against_mirror(eng, V, idx, taken, "fp32 sampled")
    assert all(np.isfinite(lp.cpu().numpy()).all() for lp in eng.last_logprobs)


def _forced(cfg, B, ends, steps, seed):
    """random forced tokens, row b forced to EOS at step ends[b]"""
    from gsv import synthetic as S
    V = cfg["model"]["vocab_size"]
    ft = torch.from_numpy(S.hash_ints("lp_force", B * steps, V - 1, seed).reshape(B, steps).astype(np.int64))
    for b, e in enumerate(ends):
        ft[b, e] = V - 1
    return ft


def test_fp32_forced_rows_finish_at_different_steps(small):
    cfg, eng = small
    B, V, steps = 5, cfg["model"]["vocab_size"], 20
    xd, bd, pd = _inputs(cfg, B, seed=29)
    ends = [3, 9, 14, 19, 0]                                # row 4: EOS forced at step 0, where the sampler masks it
    ft = _forced(cfg, B, ends, steps, seed=5)
    kw = dict(top_k=15, top_p=1.0, temperature=1.0, early_stop_num=steps - 1, repetition_penalty=1.35, seed=3)
    ys, idx = eng.infer_panel_batch_infer(xd, None, pd, bd, dump_logits=True, logprobs=True, force_tokens=ft, **kw)
    assert idx == ends
    taken = [[int(ft[b, s]) for s in range(idx[b] + 1)] for b in range(B)]
    _check_against_mirror(eng, V, idx, taken, "fp32 forced")
    assert np.isneginf(eng.last_logprobs[4].cpu().numpy()).all() and eng.last_logprobs[4].numel() == 1
    assert all(np.isfinite(eng.last_logprobs[b].cpu().numpy()).all() for b in range(4))


@pytest.mark.parametrize("B", [3, 33])
def test_fp16_engine_every_step_matches_the_mirror(v2, B):
    cfg, eng = v2
    V, steps = cfg["model"]["vocab_size"], 24
    xd, bd, pd = _inputs(cfg, B, seed=40 + B)
    kw = dict(top_k=15, top_p=1.0, temperature=1.0, early_stop_num=steps - 1, repetition_penalty=1.35, seed=11)
    ys, idx = eng.infer_panel_batch_infer(xd, None, pd, bd, dump_logits=True, logprobs=True, **kw)
    assert eng.decode_info()[0] == 1 and eng.engine_stats()[1] == 0, "the persistent engine must run"
    assert idx == [steps - 1] * B
    _check_against_mirror(eng, V, idx, _taken_sampled(eng, B, idx), f"fp16 engine B = {B}")
    # forced: rows end at different steps inside the engine launch, the rest keeps the fill
    ends = [5 + (4 * b) % 17 for b in range(B)]
    ft = _forced(cfg, B, ends, steps, seed=B)
    ys, idx = eng.infer_panel_batch_infer(xd, None, pd, bd, dump_logits=True, logprobs=True, force_tokens=ft, **kw)
    assert eng.decode_info()[0] == 1 and idx == ends
    _check_against_mirror(eng, V, idx, [[int(ft[b, s]) for s in range(idx[b] + 1)] for b in range(B)],
                          f"fp16 engine forced B = {B}")


def _tokens(out):
    ys, idx = out
    return [y.tolist() for y in ys], idx


@pytest.mark.parametrize("which", ["fp32", "fp16"])
def test_logprobs_do_not_change_the_sampling(small, v2, which):
    cfg, eng = small if which == "fp32" else v2
    B = 5 if which == "fp32" else 33
    xd, bd, pd = _inputs(cfg, B, seed=51)
    base = dict(top_k=15, top_p=0.9, temperature=0.8, early_stop_num=20, repetition_penalty=1.35)
    variants = [dict(seed=9), dict(seed=9, row_sampling=[FOUR[b % 4] for b in range(B)]),
                dict(rng_keys=[(300 + 7 * b, (3 * b + 1) % 6) for b in range(B)])]
    for v in variants:
        off = _tokens(eng.infer_panel_batch_infer(xd, None, pd, bd, **base, **v))
        assert eng.last_logprobs is None
        on = _tokens(eng.infer_panel_batch_infer(xd, None, pd, bd, logprobs=True, **base, **v))
        assert eng.decode_info()[0] == (0 if which == "fp32" else 1)
        assert on == off, f"log-probabilities changed the decode with {sorted(v)}"
        assert [lp.numel() for lp in eng.last_logprobs] == [n + 1 for n in on[1]]


@pytest.mark.parametrize("which", ["fp32", "fp16"])
def test_the_hook_holds_for_one_decode(small, v2, which):
    cfg, eng = small if which == "fp32" else v2
    B = 5
    xd, bd, pd = _inputs(cfg, B, seed=61)
    kw = dict(top_k=15, top_p=1.0, temperature=1.0, early_stop_num=12, repetition_penalty=1.35, seed=4)
    eng.infer_panel_batch_infer(xd, None, pd, bd, logprobs=True, **kw)
    buf = eng.last_logprob_buffer
    assert torch.isfinite(buf[:, 0]).all()
    buf.fill_(7.0)
    torch.cuda.synchronize()
    eng.infer_panel_batch_infer(xd, None, pd, bd, **kw)
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all()), "a plain decode wrote into the last decode's log-probability buffer"


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).tolist()


def _one_shot(eng, xd, bd, pd, keys, kw):
    ys, idx = eng.infer_panel_batch_infer(xd, None, pd, bd, rng_keys=keys, logprobs=True, **kw)
    return [y.tolist() for y in ys], idx, [_bits(lp) for lp in eng.last_logprobs], list(eng.last_cut)


def _session(eng, xd, bd, pd, keys, kw, chunk):
    B = len(xd)
    rows = [dict(x=xd[b], bert=bd[b], prompt=pd[b], key=keys[b], sampling=None) for b in range(B)]
    ys, idx, lps, cuts = [None] * B, [None] * B, [None] * B, [None] * B
    with eng.open_session(B, logprobs=True, **kw) as ses:
        assert ses.admit(rows) == list(range(B))
        calls = 0
        while ses.live:
            for t, y, n in ses.advance(chunk):
                ys[t], idx[t], lps[t], cuts[t] = y.tolist(), n, _bits(ses.logprobs[t]), ses.cut[t]
            calls += 1
            assert calls <= 100
        modes = set(ses.modes)
    return ys, idx, lps, cuts, modes


@pytest.mark.parametrize("chunk", [1, 7])
def test_fp32_session_rows_equal_the_one_shot_decode(small, chunk):
    cfg, eng = small
    B = 6
    xd, bd, pd = _inputs(cfg, B, seed=23)
    keys = [(1000 + 7 * b, (3 * b + 1) % 6) for b in range(B)]
    kw = dict(top_k=15, top_p=1.0, temperature=1.0, early_stop_num=22, repetition_penalty=1.35)
    ref = _one_shot(eng, xd, bd, pd, keys, kw)
    ys, idx, lps, cuts, modes = _session(eng, xd, bd, pd, keys, kw, chunk)
    assert modes == {0}
    assert (ys, idx, lps, cuts) == ref


def test_fp16_session_rows_equal_the_one_shot_decode(v2):
    cfg, eng = v2
    B = 33
    xd, bd, pd = _inputs(cfg, B, seed=71)
    keys = [(500 + b, b % 5) for b in range(B)]
    kw = dict(top_k=15, top_p=1.0, temperature=1.0, early_stop_num=20, repetition_penalty=1.35)
    ref = _one_shot(eng, xd, bd, pd, keys, kw)
    assert eng.decode_info()[0] == 1
    ys, idx, lps, cuts, modes = _session(eng, xd, bd, pd, keys, kw, 8)
    assert modes == {1} and eng.engine_stats()[1] == 0
    assert (ys, idx, lps, cuts) == ref
    assert all(ref[3]), "suppress_eos: every row is ended by the step budget"


def test_an_admission_leaves_the_neighbours_entries_untouched(small):
    cfg, eng = small
    B = 3
    xd, bd, pd = _inputs(cfg, B, seed=83)
    keys = [(40 + b, b) for b in range(B)]
    kw = dict(top_k=15, top_p=1.0, temperature=1.0, early_stop_num=16, repetition_penalty=1.35)
    ref = _one_shot(eng, xd, bd, pd, keys, kw)
    rows = [dict(x=xd[b], bert=bd[b], prompt=pd[b], key=keys[b], sampling=None) for b in range(B)]
    got = {}
    with eng.open_session(4, logprobs=True, **kw) as ses:
        ses.admit(rows[:2])
        for t, y, n in ses.advance(3):
            got[t] = (y.tolist(), n, _bits(ses.logprobs[t]))
        before = _bits(ses.logp[[0, 1, 3]])
        ses.admit(rows[2:], slots=[2])
        torch.cuda.synchronize()
        assert _bits(ses.logp[[0, 1, 3]]) == before, "the admission wrote into another slot's entries"
        assert bool(torch.isnan(ses.logp[3]).all()) and bool(torch.isnan(ses.logp[2, 1:]).all())
        assert _bits(ses.logp[2, :1]) == ref[2][2][:1], "step 0 of the admitted row"
        while ses.live:
            for t, y, n in ses.advance(5):
                got[t] = (y.tolist(), n, _bits(ses.logprobs[t]))
    for b in range(B):
        assert got[b] == (ref[0][b], ref[1][b], ref[2][b]), f"row {b}"
