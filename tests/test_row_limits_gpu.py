"""GPU: per-row EOS horizon, early stop and step budget in the AR decode (gsv_t2s_set_row_limits), and prompt-free rows in a
ragged batch.

Random weights never emit EOS, so the rows decode through a small model whose EOS row of ar_predict_layer is scaled up; the
CPU oracle first confirms that the input shows the horizon (under horizon 1 at least two rows end by EOS before step 11,
under horizon 11 the same rows run past step 10) before any device work.

* fp32 launch path, 6 rows with different prompt lengths (one P_b = 0) and six different limit tuples: ids, out_len and
  log-probabilities of every row are bit-equal to the row decoded alone with its limits as the call's scalars (the unchanged
  path), greedy and sampled; the greedy ids are the oracle's wherever its top-2 margin is clear;
* fp16 persistent engine, a 2-layer model of the v1/v2 shape, B = 8 (one quad) and B = 40 (pipelined quads): mixed against
  alone, mode 1, no fallback, on rows whose oracle top-2 margins are all clear of fp16 noise (V2_CLEAR, checked on the CPU);
  and on the full 24-layer model, 20 rows (one quad) and 34 rows (pipelined), every row of the mixed decode against the same
  batch decoded with that row's limits as the scalars, i.e. the same kernel with the rows' limits against itself with the
  call's scalars in every row's entry, where the bits must agree whatever the margins are;
* housekeeping: B copies of the scalars = no limits, limits hold for one call, bad values / wrong B refused, P_b = 0 without
  limits refused with today's message;
* session: 9 rows through 4 slots in chunks of 1, 3 and 7 steps equal their one-shot decodes, a reused slot keeps nothing of
  its last row's limits, and an admission leaves its neighbours' K/V and state alone.
"""
import ctypes as C

import pytest
import torch

from oracle import cases
from test_t2s_ragged_gpu import DEV, _dev, _engine, _rows

pytestmark = pytest.mark.gpu
LIMITS = [(1, -1, 40), (11, -1, 40), (1, 12, 40), (11, 5, 40), (1, -1, 7), (3, 20, 24)]
PLENS = (1, 37, 20, 9, 5, 3)
ERR_ARG = -1                      # GSV_ERR_ARG (include/gsv.h)
FREE_ROW = 4                      # the row with P_b = 0
EOS_GAIN, ROW_SEED = 4.0, 0       # chosen on the CPU: the oracle check of `small` holds for them
V2_EOS_GAIN = -8.0 # likewise for the model of the v1/v2 shape (its EOS logit is negative on these rows: the sign flips it)
GREEDY = dict(top_k=1, top_p=1.0, temperature=1.0, repetition_penalty=1.35)
SAMPLED = dict(top_k=15, top_p=1.0, temperature=1.0, repetition_penalty=1.35)


def _err(l):
    return l.gsv_last_error().decode(errors="replace")


def _eos_prone(sd, vocab, gain):
    sd = dict(sd)
    w = sd["ar_predict_layer.weight"].clone()
    w[vocab - 1] *= gain
    sd["ar_predict_layer.weight"] = w
    return sd


def _case(cfg, B, seed):
    """B rows, limits cycling through LIMITS, prompts through PLENS; every row with PLENS index FREE_ROW is prompt-free"""
    xs, berts, prompts = _rows(cfg, B, seed=seed, zh_bert=False, plens=PLENS)
    prompts = [None if b % len(PLENS) == FREE_ROW else p for b, p in enumerate(prompts)]
    return xs, berts, prompts, [LIMITS[b % len(LIMITS)] for b in range(B)], [(900 + 13 * b, b % 5) for b in range(B)]


def _alone(eng, x, bert, prompt, lim, key, kw):
    """the row decoded alone on the unchanged path: its limits as the call's scalars"""
    eos, es, ms = lim
    y, i = eng._run([x.to(DEV)], None if prompt is None else [prompt.to(DEV)], [bert.to(DEV)], kw["top_k"], kw["top_p"], es,
                    kw["temperature"], kw["repetition_penalty"], eos_mask_steps=eos, max_steps=ms, rng_keys=[key], logprobs=True)
    return y[0].cpu(), i[0], eng.last_logprobs[0].cpu().clone()


def _mixed(eng, xs, berts, prompts, lims, keys, kw, **more):
    xd, bd = _dev(xs, berts)
    pd = [None if p is None else p.to(DEV) for p in prompts]
    y, i = eng._run(xd, pd, bd, kw["top_k"], kw["top_p"], -1, kw["temperature"], kw["repetition_penalty"], eos_mask_steps=1,
                    max_steps=max(l[2] for l in lims), rng_keys=keys, row_limits=lims, logprobs=True, **more)
    return [t.cpu() for t in y], i, [t.cpu().clone() for t in eng.last_logprobs]


def _oracle_row(orc, x, bert, prompt, lim, trace=None):
    eos, es, ms = lim
    p = torch.zeros(1, 0, dtype=torch.long) if prompt is None else prompt.unsqueeze(0)
    y, i = orc.infer_panel_batch_infer([x], None, p, [bert], early_stop_num=es, eos_mask_steps=eos, max_steps=ms, trace=trace, **GREEDY)
    return y[0], i[0]


@pytest.fixture(scope="module")
def small():
    """(cfg, EOS-prone state dict, fp32 engine, the 6-row case, the oracle's per-row results under the rows' limits)"""
    from oracle.t2s_oracle import T2SOracle, apply_repetition_penalty
    cfg, sd, *_ = cases.t2s_case_inputs(cases.T2S_CASES["t2s_small_greedy"])
    sd = _eos_prone(sd, cfg["model"]["vocab_size"], EOS_GAIN)
    case = _case(cfg, 6, ROW_SEED)
    xs, berts, prompts, lims, _ = case
    threads = torch.get_num_threads()
    torch.set_num_threads(1)          # 128-wide layers: a thread pool only adds wake-ups
    try:
        orc = T2SOracle(sd, cfg)
        # is the input good?  (a failure here is a bad input -- pick another seed or gain -- not a parity failure)
        h1 = [_oracle_row(orc, xs[b], berts[b], prompts[b], (1, -1, 40))[1] for b in range(6)]
        h11 = [_oracle_row(orc, xs[b], berts[b], prompts[b], (11, -1, 40))[1] for b in range(6)]
        early = [b for b in range(6) if h1[b] < 11 and h1[b] < 39]
        assert len(early) >= 2 and all(h11[b] > 10 for b in early), f"bad input: horizon 1 ends {h1}, horizon 11 ends {h11}"
        want = []
        for b in range(6):
            tr = {}
            y, i = _oracle_row(orc, xs[b], berts[b], prompts[b], lims[b], trace=tr)
            P = 0 if prompts[b] is None else prompts[b].numel()
            full = torch.cat([y, torch.zeros(1, dtype=torch.long)])   # the finishing step's history is y itself
            clear = 0                                                # steps whose penalised top-2 margin is clear, from step 0 on
            for s, lg in enumerate(tr["logits"]):
                top2 = torch.topk(apply_repetition_penalty(lg[:1].clone(), full[:P + s].unsqueeze(0), GREEDY["repetition_penalty"])[0], 2).values
                if float(top2[0] - top2[1]) <= 1e-3:
                    break
                clear += 1
            want.append((y, i, clear, len(tr["logits"])))
    finally:
        torch.set_num_threads(threads)
    return cfg, sd, _engine(cfg, sd, torch.float32, max_batch=16, max_seq=320), case, want


def test_fp32_mixed_limits_equal_each_row_alone_and_the_oracle(small):
    cfg, sd, eng, (xs, berts, prompts, lims, keys), want = small
    for kw in (GREEDY, SAMPLED):
        ys, idx, lps = _mixed(eng, xs, berts, prompts, lims, keys, kw)
        for b in range(6):
            y1, i1, lp1 = _alone(eng, xs[b], berts[b], prompts[b], lims[b], keys[b], kw)
            print(f"[row limits] top_k {kw['top_k']} row {b} P_b {0 if prompts[b] is None else prompts[b].numel()} limits {lims[b]}: "
                  f"{idx[b]} tokens mixed, {i1} alone")
            assert idx[b] == i1 and ys[b].tolist() == y1.tolist(), f"row {b} {lims[b]}: mixed decode differs from the row alone"
            assert lps[b].shape == lp1.shape and torch.equal(lps[b].view(torch.int32), lp1.view(torch.int32)), \
                f"row {b}: log-probabilities differ from the row alone"
            assert idx[b] <= min(lims[b][2], lims[b][1] + 1 if lims[b][1] >= 0 else lims[b][2]) - 1
        if kw is GREEDY:
            for b, (oy, oi, clear, nsteps) in enumerate(want):
                P = 0 if prompts[b] is None else prompts[b].numel()
                if clear == nsteps:
                    assert idx[b] == oi and ys[b].tolist() == oy.tolist(), f"row {b} {lims[b]} differs from the oracle"
                else:
                    n = min(clear, idx[b], oi)
                    assert ys[b][:P + n].tolist() == oy[:P + n].tolist(), f"row {b} leaves the oracle on a clear margin"
    assert len({i for i in idx}) > 1


def test_scalars_as_limits_are_the_scalar_decode_and_limits_hold_one_call(small):
    cfg, sd, eng, (xs, berts, prompts, lims, keys), _ = small
    rows = [b for b in range(6) if prompts[b] is not None]
    x, bt, p, k = ([a[b] for b in rows] for a in (xs, berts, prompts, keys))
    xd, bd = _dev(x, bt)
    pd = [q.to(DEV) for q in p]
    s = SAMPLED

    def scalar():
        y, i = eng._run(xd, pd, bd, s["top_k"], s["top_p"], 12, s["temperature"], s["repetition_penalty"], eos_mask_steps=3,
                        max_steps=30, rng_keys=k, logprobs=True)
        return [t.tolist() for t in y], i, [t.cpu().clone() for t in eng.last_logprobs]
    y0, i0, l0 = scalar()
    y1, i1 = eng._run(xd, pd, bd, s["top_k"], s["top_p"], 12, s["temperature"], s["repetition_penalty"], eos_mask_steps=3,
                      max_steps=30, rng_keys=k, logprobs=True, row_limits=[(3, 12, 30)] * len(rows))
    l1 = [t.cpu().clone() for t in eng.last_logprobs]
    assert i0 == i1 and y0 == [t.tolist() for t in y1]
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(l0, l1))
    # other limits change the decode, and are gone with the call that used them
    y2, i2 = eng._run(xd, pd, bd, s["top_k"], s["top_p"], 12, s["temperature"], s["repetition_penalty"], eos_mask_steps=3,
                      max_steps=30, rng_keys=k, row_limits=[(3, 4, 30)] * len(rows))
    assert i2 == [4] * len(rows) and i2 != i0
    y3, i3, l3 = scalar()
    assert (y3, i3) == (y0, i0)


def test_bad_limits_and_prompt_free_rows_without_limits_are_refused(small):
    from gsv import _lib
    cfg, sd, eng, (xs, berts, prompts, lims, keys), _ = small
    l = _lib.lib()

    def set_limits(rows):
        arr = (_lib.RowLimits * len(rows))(*[_lib.RowLimits(*r) for r in rows])
        return l.gsv_t2s_set_row_limits(eng._h, arr, len(rows))
    for bad in [(-1, -1, 8, 0), (1, -2, 8, 0), (1, -1, 0, 0), (1, -1, 8, 1)]:
        assert set_limits([(1, -1, 8, 0), bad]) == ERR_ARG, bad
    assert l.gsv_t2s_set_row_limits(eng._h, None, 2) == ERR_ARG
    assert l.gsv_t2s_set_row_limits(eng._h, (_lib.RowLimits * 1)(), 0) == ERR_ARG
    # nothing was kept: a prompt-free row in a ragged batch is still refused, with the message of the parent commit
    xd, bd = _dev(xs[:2], berts[:2])
    phones = torch.cat([t.reshape(-1) for t in xd]).to(torch.int32)
    lens = (C.c_int32 * 2)(*[int(t.numel()) for t in xd])
    pr = prompts[0].to(DEV, torch.int32)
    plens = (C.c_int32 * 2)(int(pr.numel()), 0)
    torch.cuda.synchronize()

    def prefill():
        return l.gsv_t2s_prefill_ragged(eng._h, phones.data_ptr(), C.cast(lens, C.c_void_p), 2, None, pr.data_ptr(),
                                        C.cast(plens, C.c_void_p), None)
    assert prefill() == ERR_ARG
    assert "row 1 has prompt length 0 (must be >= 1)" in _err(l)
    with pytest.raises(ValueError, match="at least one token"):
        eng._run(xd, [prompts[0].to(DEV), None], bd, 1, 1.0, -1, 1.0, 1.35, eos_mask_steps=1, max_steps=8)
    # a wrong B is refused by the prefill and by the decode, before any launch, and the limits are dropped
    assert set_limits([(1, -1, 8, 0)] * 3) == 0
    assert prefill() == ERR_ARG and "3 rows for a batch of 2" in _err(l)
    assert prefill() == ERR_ARG and "must be >= 1" in _err(l)
    pr2 = torch.cat([prompts[0], prompts[1]]).to(DEV, torch.int32)
    plens2 = (C.c_int32 * 2)(int(prompts[0].numel()), int(prompts[1].numel()))

    def prefill2():
        torch.cuda.synchronize()
        return l.gsv_t2s_prefill_ragged(eng._h, phones.data_ptr(), C.cast(lens, C.c_void_p), 2, None, pr2.data_ptr(),
                                        C.cast(plens2, C.c_void_p), None)
    assert prefill2() == 0
    out_tokens = torch.zeros(2, 8, dtype=torch.int32, device=DEV)
    out_len = torch.full((2,), -7, dtype=torch.int32, device=DEV)
    sp = _lib.SamplingParams(1, 1.0, 1.0, 1.35, -1, 1, 8, 0)
    steps = C.c_int(0)

    def decode():
        torch.cuda.synchronize()
        return l.gsv_t2s_decode(eng._h, C.byref(sp), None, 0, out_tokens.data_ptr(), out_len.data_ptr(), C.byref(steps), None)
    assert set_limits([(1, -1, 8, 0)] * 3) == 0
    assert decode() == ERR_ARG and "3 rows for a batch of 2" in _err(l)
    assert set_limits([(1, -1, 8, 0), (1, -1, 9, 0)]) == 0              # above the call's max_steps
    assert decode() == ERR_ARG and "exceed the call's 8" in _err(l)
    torch.cuda.synchronize()
    assert out_len.tolist() == [-7, -7] and int(out_tokens.abs().sum()) == 0, "a refused decode must not launch"
    assert prefill2() == 0 and decode() == 0                            # the limits went with the refused call
    torch.cuda.synchronize()
    assert min(out_len.tolist()) >= 0


# Two fp16 kernels that compute the same sums in another order (the pipelined engine kernel for B > 32, the single-quad one for
# a row alone) may round an activation to the neighbouring fp16 value, so their greedy ids agree only where the top-2 margin of
# the logits is clear of that noise.  The project holds the 24-layer engine's logits to 5e-2 of the fp32 ones
# (test_t2s_ragged_gpu.py); the noise of independent roundings grows with the square root of their number, about five per
# layer plus the logits GEMM, so a 2-layer model of the same shape is held to 5e-2 * sqrt(11 / 121) = 1.5e-2, and two kernels
# inside that band differ by at most 3e-2.  The rows of the fp16 cases are therefore chosen ON THE CPU, from the oracle's
# fp32 logits alone: a case whose smallest penalised top-2 margin over every step of every row is not above V2_CLEAR is a bad
# input (another seed), checked before any device work like the horizon.  (On the 24-layer model no such input exists: rows of
# 39 steps meet margins below 1e-2 every few rows, and 5 of 34 rows of a default batch, no limits set, left their alone decode
# at margins of 0.0006 .. 0.005.)
V2_LAYERS, V2_CLEAR = 2, 3e-2
V2_SEED = {8: 339, 40: 339}      # found by scanning seeds with the oracle; nothing was run on a GPU to pick them


@pytest.fixture(scope="module")
def v2_prone():
    """(2-layer config of the v1/v2 shape, EOS-prone state dict, fp16 engine, {B: the case, its oracle margin checked})"""
    import copy
    from gsv import synthetic as S
    from oracle.t2s_oracle import T2SOracle, apply_repetition_penalty
    cfg = copy.deepcopy(S.T2S_V2_CONFIG)
    cfg["model"]["n_layer"] = V2_LAYERS
    sd = _eos_prone(S.make_t2s_state_dict(cfg, seed=0), cfg["model"]["vocab_size"], V2_EOS_GAIN)
    orc = T2SOracle(sd, cfg)
    cases_ = {}
    for B, seed in V2_SEED.items():
        case = _case(cfg, B, seed=seed)
        xs, berts, prompts, lims, _ = case
        worst = float("inf")
        for b in range(B):
            tr = {}
            y, i = _oracle_row(orc, xs[b], berts[b], prompts[b], lims[b], trace=tr)
            P = 0 if prompts[b] is None else prompts[b].numel()
            for s, lg in enumerate(tr["logits"]):
                top2 = torch.topk(apply_repetition_penalty(lg[:1].clone(), y[:P + s].unsqueeze(0), GREEDY["repetition_penalty"])[0], 2).values
                worst = min(worst, float(top2[0] - top2[1]))
        assert worst > V2_CLEAR, f"bad input: B = {B} seed {seed} has a top-2 margin of {worst:.4f} in the oracle"
        cases_[B] = case
    # the horizon shows: under horizon 1 at least two rows end by EOS before step 11, under horizon 11 the same rows run past 10
    xs, berts, prompts, _, _ = cases_[8]
    h1 = [_oracle_row(orc, xs[b], berts[b], prompts[b], (1, -1, 14))[1] for b in range(6)]
    h11 = [_oracle_row(orc, xs[b], berts[b], prompts[b], (11, -1, 14))[1] for b in range(6)]
    assert sum(a < 11 and c > 10 for a, c in zip(h1, h11)) >= 2, f"bad input: horizon 1 ends {h1}, horizon 11 ends {h11}"
    return cfg, sd, _engine(cfg, sd, torch.float16, max_batch=40, max_seq=256), cases_


@pytest.mark.parametrize("B", [8, 40])
def test_fp16_engine_mixed_limits_equal_each_row_alone(v2_prone, B):
    """B = 40 compares the pipelined kernel (the batch) with the single-quad kernel (a row alone): see V2_CLEAR above for the
    inputs on which two fp16 kernels can be held to the same ids."""
    cfg, sd, eng, cases_ = v2_prone
    xs, berts, prompts, lims, keys = cases_[B]
    ys, idx, _ = _mixed(eng, xs, berts, prompts, lims, keys, GREEDY)
    assert eng.decode_info()[0] == 1, "the persistent engine must run the decode with limits"
    for b in range(B):
        y1, i1, _ = _alone(eng, xs[b], berts[b], prompts[b], lims[b], keys[b], GREEDY)
        assert eng.decode_info()[0] == 1
        assert idx[b] == i1 and ys[b].tolist() == y1.tolist(), f"row {b} {lims[b]}: {idx[b]} tokens mixed, {i1} alone"
    print(f"[row limits] fp16 engine B = {B}: tokens per row {idx}")
    assert eng.engine_stats()[1] == 0
    assert len(set(idx)) > 2, "the limits must show in the rows' lengths"


@pytest.fixture(scope="module")
def v2_full():
    """the full 24-layer T2S_V2_CONFIG with the EOS-prone head, fp16 engine: for the comparison that no margin touches"""
    from gsv import synthetic as S
    cfg = S.T2S_V2_CONFIG
    sd = _eos_prone(S.make_t2s_state_dict(cfg, seed=0), cfg["model"]["vocab_size"], V2_EOS_GAIN)
    return cfg, sd, _engine(cfg, sd, torch.float16, max_batch=40, max_seq=256)


@pytest.mark.parametrize("B", [24, 40])
def test_fp16_engine_with_limits_equals_the_scalar_decode_of_the_same_batch(v2_full, B):
    """Full-size engine, single-quad (20 rows) and pipelined (34 rows) kernel: every row of the decode with limits against the
    SAME batch decoded with that row's limits as the scalars -- the same kernel, reading the rows' own limits in one decode and
    the call's scalars from every row's entry in the other, the same sums in the same order, so the bits must agree whatever the
    margins are."""
    cfg, sd, eng = v2_full
    xs, berts, prompts, lims, keys = _case(cfg, B, seed=41)
    rows = [b for b in range(B) if prompts[b] is not None]           # the scalar path takes no prompt-free row in a ragged batch
    xs, berts, prompts, lims, keys = ([a[b] for b in rows] for a in (xs, berts, prompts, lims, keys))
    ys, idx, _ = _mixed(eng, xs, berts, prompts, lims, keys, SAMPLED)
    assert eng.decode_info()[0] == 1 and (len(rows) > 32) == (B == 40)
    xd, bd = _dev(xs, berts)
    pd = [p.to(DEV) for p in prompts]
    s = SAMPLED
    for eos, es, ms in sorted(set(lims)):
        y, i = eng._run(xd, pd, bd, s["top_k"], s["top_p"], es, s["temperature"], s["repetition_penalty"], eos_mask_steps=eos,
                        max_steps=ms, rng_keys=keys)
        assert eng.decode_info()[0] == 1
        for b in range(len(rows)):
            if lims[b] == (eos, es, ms):
                assert idx[b] == i[b] and ys[b].tolist() == y[b].cpu().tolist(), f"row {b} {lims[b]}: {idx[b]} tokens, scalar batch {i[b]}"
    assert eng.engine_stats()[1] == 0


def test_session_rows_with_limits_equal_their_one_shot_decodes(small):
    cfg, sd, eng, _, _ = small
    N, slots = 9, 4
    xs, berts, prompts, lims, keys = _case(cfg, N, seed=3)
    kw = SAMPLED
    want = [_alone(eng, xs[b], berts[b], prompts[b], lims[b], keys[b], kw) for b in range(N)]
    rows = [dict(x=xs[b].to(DEV), bert=berts[b].to(DEV), prompt=None if prompts[b] is None else prompts[b].to(DEV), key=keys[b],
                 limits=lims[b]) for b in range(N)]
    got, where, lim_of_slot = {}, {}, {}
    with eng.open_session(slots, kw["top_k"], kw["top_p"], kw["temperature"], kw["repetition_penalty"], -1, eos_mask_steps=1,
                          max_steps=40, row_limits=True, logprobs=True) as ses:
        q, chunks, turn = 0, (1, 3, 7), 0
        while q < N or ses.live:
            k = min(len(ses.free), N - q, 1 + turn % 2)            # staggered: one or two rows per admission
            if k:
                busy = [s for s in range(slots) if s not in ses.free]
                before = ses.state().copy()
                kv = {s: [eng.debug_kv(layer, w, s, int(before[0, s])).clone() for layer in (0, 1) for w in (0, 1)] for s in busy}
                for t, b in zip(ses.admit(rows[q:q + k]), range(q, q + k)):
                    where[t] = b
                after = ses.state()
                for s in busy:                                      # the neighbours: state and K/V untouched
                    assert (before[:, s] == after[:, s]).all(), f"admission changed the state of slot {s}"
                    now = [eng.debug_kv(layer, w, s, int(before[0, s])) for layer in (0, 1) for w in (0, 1)]
                    assert all(torch.equal(a, b_) for a, b_ in zip(kv[s], now)), f"admission changed the K/V of slot {s}"
                q += k
            for t, y, n in ses.advance(chunks[turn % 3]):
                got[where[t]] = (y.cpu(), n, ses.logprobs[t].cpu(), ses.cut[t])
            turn += 1
        for t, s in ses.history:
            lim_of_slot.setdefault(s, []).append(lims[where[t]])
    assert any(len(set(v)) > 1 for v in lim_of_slot.values()), "no slot was reused by a row with other limits"
    for b in range(N):
        y1, i1, lp1 = want[b]
        y, n, lp, cut = got[b]
        assert n == i1 and y.tolist() == y1.tolist(), f"row {b} {lims[b]}: session {n} tokens, one-shot {i1}"
        assert torch.equal(lp.view(torch.int32), lp1.view(torch.int32))
        eos, es, ms = lims[b]
        assert cut == (n >= min(ms, es + 1 if es >= 0 else ms) - 1)
    # a session that is opened without the flag refuses limits and prompt-free rows, and decodes as before
    with eng.open_session(slots, kw["top_k"], kw["top_p"], kw["temperature"], kw["repetition_penalty"], -1, max_steps=40) as ses:
        with pytest.raises(ValueError, match="row_limits=True"):
            ses.admit(rows[:1])
