"""GPU: the AR decode's row tables.  Every row samples and stops by its own entry of the device tables (sampling values, limits,
counter-RNG key); a call that brings no rows of its own has the tables filled with its scalars.  What can go wrong is a stale
entry: a row that decodes by what the table held for an earlier call or an earlier session.

* one-shot decodes: on one handle B1 rows decode with per-row sampling values and per-row limits, all different and none
  greedy; then B2 < B1 rows decode with scalars only, greedy and sampled, which differ from what the rows' entries held.  Ids,
  out_len and log-probability bits of the second decode equal the same decode on a fresh handle.  fp32 small model on the launch
  path (5 then 3 rows) and the 2-layer fp16 model of the v1/v2 shape on the persistent engine: 8 then 6 rows (single-quad
  kernel), 40 then 34 rows (pipelined kernel).  The EOS-prone head of test_row_limits_gpu.py makes the rows end at different
  steps; the CPU oracle confirms that for the greedy scalar decode before any device work (and, for fp16, that its top-2
  margins are clear of fp16 noise: V2_CLEAR there).
* sessions: a session opened without row_sampling that is never given limits, six rows staggered through 4 slots, equals the
  rows' one-shot scalar decodes although every slot's last occupant, in an earlier session of the same handle, had sampling
  values and limits of its own.  The scalars mask EOS for 11 of the 12 steps, so every row outlives the stale budgets.
"""
import copy

import pytest
import torch

from oracle import cases
from test_row_limits_gpu import EOS_GAIN, GREEDY, PLENS, SAMPLED, V2_CLEAR, V2_EOS_GAIN, V2_LAYERS, _eos_prone, _oracle_row
from test_t2s_ragged_gpu import DEV, _dev, _engine, _rows

pytestmark = pytest.mark.gpu
SCALAR_LIMITS = (1, -1, 12)                      # eos_mask_steps, early_stop_num, max_steps of the scalar decodes
CASES = {("small", 5, 3): 74, ("v2", 8, 6): 3, ("v2", 40, 34): 43}   # (model, B1, B2): the seed of its rows, chosen on the CPU
                                                                     # with the oracle (_scalar_case); nothing ran on a GPU for it


def _row_tables(B):
    """per-row sampling values and limits, all different, none greedy, none equal to the scalars, budgets of 4 .. 10 steps"""
    sampling = [(5 + b, 0.85 if b % 2 else 1.0, 0.7 + 0.01 * b, 1.1 + 0.01 * b) for b in range(B)]
    limits = [(1 + b % 5, 3 + b % 7, 5 + b % 8) for b in range(B)]
    assert len(set(sampling)) == B and len(set(limits)) == B
    return sampling, limits


def _scalar_case(cfg, sd, B1, B2, seed, clear):
    """B1 rows, and the oracle's check that the first B2 of them are a good input for the greedy scalar decode: they end at
    different steps, one of them after the budget and one before the EOS horizon that _row_tables left in its table entry, and
    every penalised top-2 margin is above `clear`"""
    from oracle.t2s_oracle import T2SOracle, apply_repetition_penalty
    xs, berts, prompts = _rows(cfg, B1, seed=seed, zh_bert=False, plens=PLENS)
    orc = T2SOracle(sd, cfg)
    ends, worst = [], float("inf")
    for b in range(B2):
        tr = {}
        y, i = _oracle_row(orc, xs[b], berts[b], prompts[b], SCALAR_LIMITS, trace=tr)
        ends.append(i)
        full = torch.cat([y, torch.zeros(1, dtype=torch.long)])
        for s, lg in enumerate(tr["logits"]):
            top2 = torch.topk(apply_repetition_penalty(lg[:1].clone(), full[:prompts[b].numel() + s].unsqueeze(0),
                                                       GREEDY["repetition_penalty"])[0], 2).values
            worst = min(worst, float(top2[0] - top2[1]))
    stale = _row_tables(B1)[1]
    outlives = [b for b in range(B2) if ends[b] > min(stale[b][2], stale[b][1] + 1) - 1]
    masked = [b for b in range(B2) if ends[b] < stale[b][0] and ends[b] < SCALAR_LIMITS[2] - 1]
    assert len(set(ends)) > 1 and outlives and masked and worst > clear, \
        f"bad input: seed {seed} ends {ends}, smallest top-2 margin {worst:.4f}"
    return xs, berts, prompts, ends


def _models():
    from gsv import synthetic as S
    cfg, sd, *_ = cases.t2s_case_inputs(cases.T2S_CASES["t2s_small_greedy"])
    small = (cfg, _eos_prone(sd, cfg["model"]["vocab_size"], EOS_GAIN), torch.float32, 1e-3)
    cfg2 = copy.deepcopy(S.T2S_V2_CONFIG)
    cfg2["model"]["n_layer"] = V2_LAYERS
    v2 = (cfg2, _eos_prone(S.make_t2s_state_dict(cfg2, seed=0), cfg2["model"]["vocab_size"], V2_EOS_GAIN), torch.float16, V2_CLEAR)
    return {"small": small, "v2": v2}


@pytest.fixture(scope="module")
def models():
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        m = _models()
        checked = {(name, B1, B2): _scalar_case(m[name][0], m[name][1], B1, B2, seed, m[name][3])
                   for (name, B1, B2), seed in CASES.items()}
    finally:
        torch.set_num_threads(threads)
    return m, checked


def _scalar(eng, xd, pd, bd, kw):
    eos, es, ms = SCALAR_LIMITS
    y, i = eng._run(xd, pd, bd, kw["top_k"], kw["top_p"], es, kw["temperature"], kw["repetition_penalty"], eos_mask_steps=eos,
                    max_steps=ms, seed=77, logprobs=True)
    return [t.cpu().tolist() for t in y], i, [t.cpu().clone() for t in eng.last_logprobs], eng.decode_info()[0]


@pytest.mark.parametrize("name,B1,B2", list(CASES))
def test_scalar_decode_after_a_per_row_decode_reads_no_stale_entry(models, name, B1, B2):
    m, checked = models
    cfg, sd, dtype, _ = m[name]
    xs, berts, prompts, ends = checked[(name, B1, B2)]
    mode = 1 if dtype == torch.float16 else 0
    eng, fresh = (_engine(cfg, sd, dtype, max_batch=B1, max_seq=256) for _ in range(2))
    xd, bd = _dev(xs, berts)
    pd = [p.to(DEV) for p in prompts]
    sampling, limits = _row_tables(B1)
    for kw in (GREEDY, SAMPLED):
        # B1 rows by their own entries, then B2 rows by the scalars, on the same handle
        y1, i1 = eng._run(xd, pd, bd, 15, 1.0, -1, 1.0, 1.35, eos_mask_steps=1, max_steps=12, seed=5, row_sampling=sampling,
                          row_limits=limits, logprobs=True)
        assert eng.decode_info()[0] == mode
        assert all(i1[b] <= min(limits[b][2], limits[b][1] + 1) - 1 for b in range(B1))
        got = _scalar(eng, xd[:B2], pd[:B2], bd[:B2], kw)
        want = _scalar(fresh, xd[:B2], pd[:B2], bd[:B2], kw)
        print(f"[row tables] {name} B1 {B1} B2 {B2} top_k {kw['top_k']}: per-row decode ends {i1}, scalar decode ends {got[1]}, "
              f"fresh handle {want[1]}, oracle (greedy) {ends}")
        assert got[3] == mode and want[3] == mode
        assert got[1] == want[1] and got[0] == want[0], "the scalar decode differs from the one on a fresh handle"
        assert all(a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got[2], want[2])), \
            "the scalar decode's log-probabilities differ from the ones on a fresh handle"
        if kw is GREEDY:
            assert len(set(got[1])) > 1, "the rows must end at different steps"
    if mode == 1:
        assert eng.engine_stats()[1] == 0 and fresh.engine_stats()[1] == 0


def test_session_without_rows_of_its_own_decodes_by_its_scalars(models):
    m, _ = models
    cfg, sd, dtype, _ = m["small"]
    N, slots = 6, 4
    xs, berts, prompts = _rows(cfg, N, seed=CASES[("small", 5, 3)], zh_bert=False, plens=PLENS)
    keys = [(300 + 7 * b, b % 3) for b in range(N)]
    kw, (eos, es, ms) = SAMPLED, (11, -1, 12)
    eng, fresh = (_engine(cfg, sd, dtype, max_batch=8, max_seq=256) for _ in range(2))
    want = []
    for b in range(N):
        y, i = fresh._run([xs[b].to(DEV)], [prompts[b].to(DEV)], [berts[b].to(DEV)], kw["top_k"], kw["top_p"], es, kw["temperature"],
                          kw["repetition_penalty"], eos_mask_steps=eos, max_steps=ms, rng_keys=[keys[b]], logprobs=True)
        want.append((y[0].cpu().tolist(), i[0], fresh.last_logprobs[0].cpu().clone()))
    assert all(w[1] == ms - 1 for w in want), "EOS is masked until the last step: every row runs to the budget"
    rows = [dict(x=xs[b].to(DEV), bert=berts[b].to(DEV), prompt=prompts[b].to(DEV), key=keys[b]) for b in range(N)]
    # an earlier session of the same handle: every slot holds a row with sampling values and limits of its own
    sampling, limits = _row_tables(slots)
    with eng.open_session(slots, 15, 1.0, 1.0, 1.35, -1, eos_mask_steps=1, max_steps=ms, row_sampling=True, row_limits=True) as ses:
        ses.admit([dict(rows[b], sampling=sampling[b], limits=limits[b]) for b in range(slots)])
        while ses.live:
            for t, y, n in ses.advance(4):
                assert n <= min(limits[t][2], limits[t][1] + 1) - 1
    got, where = {}, {}
    with eng.open_session(slots, kw["top_k"], kw["top_p"], kw["temperature"], kw["repetition_penalty"], es, eos_mask_steps=eos,
                          max_steps=ms, logprobs=True) as ses:
        q, chunks, turn = 0, (1, 3, 7), 0
        while q < N or ses.live:
            k = min(len(ses.free), N - q, 1 + turn % 2)            # staggered: one or two rows per admission
            for t, b in zip(ses.admit(rows[q:q + k]) if k else [], range(q, q + k)):
                where[t] = b
            q += k
            for t, y, n in ses.advance(chunks[turn % 3]):
                got[where[t]] = (y.cpu().tolist(), n, ses.logprobs[t].cpu())
            turn += 1
        assert sorted(s for _, s in ses.history[:slots]) == list(range(slots)), "every slot of the earlier session is used again"
    for b in range(N):
        assert got[b][1] == want[b][1] and got[b][0] == want[b][0], f"row {b}: session {got[b][1]} tokens, one-shot {want[b][1]}"
        assert torch.equal(got[b][2].view(torch.int32), want[b][2].view(torch.int32)), f"row {b}: log-probabilities differ"
