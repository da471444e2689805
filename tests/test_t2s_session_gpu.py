"""GPU: AR decode sessions (gsv_t2s_session_*, Text2SemanticDecoder.open_session / infer_panel_continuous): rows are admitted
into free slots between engine launches, advanced a chunk of steps at a time, and their slots are admitted again.

1. a decode cut into chunks is the one-shot decode, bit for bit (ids, idx, per-step logits): fp32 launch path at chunks of
   1 / 7 / 40, fp16 persistent engine at B = 32 (one quad) and B = 36 (pipelined quads), and across the 320-position LDS image;
2. admission, fp32: a queue of 13 ragged rows through 4 slots gives every row the ids the oracle gives for it alone (greedy) and
   the ids an ordinary decode of the row alone with its key gives (top_k = 15, and with per-row sampling values);
3. admission, fp16 engine: 48 rows through 32 / 36 slots, teacher-forced on the fp32 ids with forced EOS so that slots are
   reused; every step's logits of every row within the 5e-2 band of test_t2s_ragged_gpu.py, every advance on the engine;
4. an admission leaves its neighbours' K/V and row state bit-identical, and a refused admission changes nothing;
5. the ordinary entry points raise while a session is open and decode what they decoded before once it is closed.
"""
import collections

import numpy as np
import pytest
import torch

from oracle import cases
from test_t2s_ragged_gpu import DEV, PLENS, _dev, _engine, _rows

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def small():
    cfg, sd, *_ = cases.t2s_case_inputs(cases.T2S_CASES["t2s_small_greedy"])
    return cfg, sd, _engine(cfg, sd, torch.float32, max_batch=64, max_seq=320)


@pytest.fixture(scope="module")
def v2():
    from gsv import synthetic as S
    cfg = S.T2S_V2_CONFIG
    return cfg, S.make_t2s_state_dict(cfg, seed=0, suppress_eos=True)


@pytest.fixture(scope="module")
def v2_f16(v2):
    cfg, sd = v2
    return _engine(cfg, sd, torch.float16, max_batch=64, max_seq=384)


def _session_rows(xd, bd, pd, keys, sampling=None):
    return [dict(x=xd[b], bert=bd[b], prompt=pd[b], key=keys[b], sampling=None if sampling is None else sampling[b])
            for b in range(len(xd))]


def _chunked(eng, rows, chunk, **kw):
    """all rows admitted at once into slots 0 .. B - 1, then advanced in chunks until every row is done"""
    B = len(rows)
    ys, idx, logits = [None] * B, [None] * B, [None] * B
    with eng.open_session(B, dump_logits=True, **kw) as ses:
        tickets = ses.admit(rows)
        assert tickets == list(range(B)) and [s for _, s in ses.history] == list(range(B))
        calls = 0
        while ses.live:
            for t, y, n in ses.advance(chunk):
                ys[t], idx[t], logits[t] = y, n, ses.logits[t]
            calls += 1
            assert calls <= 200
        modes = list(ses.modes)
    return ys, idx, logits, modes, calls


def _assert_same(eng_out, ref_y, ref_idx, ref_dump):
    ys, idx, logits = eng_out
    assert idx == ref_idx
    assert [y.tolist() for y in ys] == [y.tolist() for y in ref_y]
    for b, n in enumerate(ref_idx):
        assert torch.equal(logits[b].cpu(), ref_dump[:n + 1, b].cpu()), f"row {b}: logits differ from the one-shot decode"


# ---- 1. chunked equals one-shot, bit for bit ----

@pytest.fixture(scope="module")
def small_one_shot(small):
    cfg, sd, eng = small
    B = 9
    xs, berts, prompts = _rows(cfg, B, seed=23, zh_bert=True)
    assert len({p.numel() for p in prompts}) == len(PLENS)
    xd, bd = _dev(xs, berts)
    pd = [p.to(DEV) for p in prompts]
    keys = [(1000 + 7 * b, (3 * b + 1) % 6) for b in range(B)]
    kw = dict(top_k=15, top_p=1.0, temperature=1.0, early_stop_num=40, repetition_penalty=1.35)
    y, i = eng.infer_panel_batch_infer(xd, None, pd, bd, rng_keys=keys, dump_logits=True, **kw)
    return _session_rows(xd, bd, pd, keys), kw, y, i, eng.last_logits_dump.clone()


@pytest.mark.parametrize("chunk", [1, 7, 40])
def test_fp32_chunked_decode_is_the_one_shot_decode(small, small_one_shot, chunk):
    eng = small[2]
    rows, kw, ref_y, ref_idx, ref_dump = small_one_shot
    ys, idx, logits, modes, calls = _chunked(eng, rows, chunk, **kw)
    assert set(modes) == {0}
    assert calls == -(-max(ref_idx) // chunk), "rows resume where the last chunk left them"
    _assert_same((ys, idx, logits), ref_y, ref_idx, ref_dump)


@pytest.mark.parametrize("B", [32, 36])
def test_fp16_engine_chunked_decode_is_the_one_shot_decode(v2, v2_f16, B):
    cfg, eng = v2[0], v2_f16
    xs, berts, prompts = _rows(cfg, B, seed=B, zh_bert=True)
    xd, bd = _dev(xs, berts)
    pd = [p.to(DEV) for p in prompts]
    keys = [(500 + b, b % 5) for b in range(B)]
    kw = dict(top_k=15, top_p=1.0, temperature=1.0, early_stop_num=30, repetition_penalty=1.35)
    ref_y, ref_idx = eng.infer_panel_batch_infer(xd, None, pd, bd, rng_keys=keys, dump_logits=True, **kw)
    ref_dump = eng.last_logits_dump.clone()
    assert eng.decode_info()[0] == 1 and ref_idx == [30] * B
    ys, idx, logits, modes, calls = _chunked(eng, _session_rows(xd, bd, pd, keys), 7, **kw)
    assert modes == [1] * 5 and calls == 5, "every chunk of 7 runs on the persistent engine"
    assert eng.engine_stats()[1] == 0
    _assert_same((ys, idx, logits), ref_y, ref_idx, ref_dump)


def test_fp16_engine_chunks_on_both_sides_of_the_320_position_image(v2, v2_f16):
    cfg, eng = v2[0], v2_f16
    B, steps = 4, 20
    # 150 phonemes + 163 prompt tokens = 313 cached positions: the cache passes 320 at step 7, chunks end at steps 5 and 10
    xs, berts, prompts = _rows(cfg, B, seed=9, zh_bert=True, plens=(163,), xlo=150, xhi=151)
    assert all(x.numel() + p.numel() == 313 for x, p in zip(xs, prompts))
    xd, bd = _dev(xs, berts)
    pd = [p.to(DEV) for p in prompts]
    keys = [(77, b) for b in range(B)]
    kw = dict(top_k=15, top_p=1.0, temperature=1.0, early_stop_num=steps, repetition_penalty=1.35)
    ref_y, ref_idx = eng.infer_panel_batch_infer(xd, None, pd, bd, rng_keys=keys, dump_logits=True, **kw)
    ref_dump = eng.last_logits_dump.clone()
    assert eng.decode_info()[0] == 1 and ref_idx == [steps] * B
    ys, idx, logits, modes, calls = _chunked(eng, _session_rows(xd, bd, pd, keys), 5, **kw)
    assert modes == [1] * 4 and eng.engine_stats()[1] == 0
    _assert_same((ys, idx, logits), ref_y, ref_idx, ref_dump)


# ---- 2. admission, fp32 ----

QUEUE_SEED = 130      # chosen with the oracle: lengths {17, 24, 40}, two rows end at EOS, every slot takes three rows or more


@pytest.fixture(scope="module")
def queue13(small):
    cfg = small[0]
    xs, berts, prompts = _rows(cfg, 13, seed=QUEUE_SEED, zh_bert=True)
    xd, bd = _dev(xs, berts)
    return xs, berts, prompts, xd, bd, [p.to(DEV) for p in prompts]


def _slot_use(eng):
    return collections.Counter(s for _, s in eng.last_session.history)


def test_fp32_admitted_rows_decode_the_oracles_ids(small, queue13):
    from oracle.t2s_oracle import T2SOracle
    cfg, sd, eng = small
    xs, berts, prompts, xd, bd, pd = queue13
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, early_stop_num=40, repetition_penalty=1.35)
    ys, idxs = eng.infer_panel_continuous(xd, pd, bd, rng_keys=[(0, b) for b in range(13)], slots=4, chunk=5, admit_min=1, **kw)
    # the case is not vacuous: unequal lengths, an EOS before the cap, every slot reused at least twice
    assert len(set(idxs)) >= 3, idxs
    assert min(idxs) < 40, idxs
    use = _slot_use(eng)
    assert sorted(use) == [0, 1, 2, 3] and min(use.values()) >= 3, use
    orc = T2SOracle(sd, cfg)
    for b in range(13):
        oy, oi = orc.infer_panel_batch_infer([xs[b]], None, prompts[b].unsqueeze(0), [berts[b]], **kw)
        assert idxs[b] == oi[0], f"row {b} (P_b = {prompts[b].numel()}): {idxs[b]} tokens, oracle {oi[0]}"
        assert ys[b].cpu().tolist() == oy[0].tolist(), f"row {b} (P_b = {prompts[b].numel()}) differs from the oracle"


@pytest.mark.parametrize("per_row", [False, True])
def test_fp32_admitted_rows_draw_what_they_draw_alone(small, queue13, per_row):
    eng = small[2]
    xs, berts, prompts, xd, bd, pd = queue13
    keys = [(2000 + 11 * b, (5 * b + 2) % 7) for b in range(13)]
    base = (15, 1.0, 1.0, 1.35)
    sampling = [(15, 1.0, 1.0, 1.35), (5, 0.9, 0.8, 1.2), (0, 0.7, 1.3, 1.0), (30, 1.0, 0.6, 1.5)]
    rs = [sampling[b % 4] for b in range(13)] if per_row else None
    kw = dict(top_k=base[0], top_p=base[1], temperature=base[2], repetition_penalty=base[3], early_stop_num=40)
    ys, idxs = eng.infer_panel_continuous(xd, pd, bd, rng_keys=keys, row_sampling=rs, slots=4, chunk=5, admit_min=1, **kw)
    use = _slot_use(eng)
    assert sum(use.values()) == 13 and min(use.values()) >= 2
    assert len({tuple(y.tolist()) for y in ys}) == 13
    for b in range(13):
        k, p, t, r = rs[b] if per_row else base
        ya, ia = eng.infer_panel_batch_infer([xd[b]], None, [pd[b]], [bd[b]], top_k=k, top_p=p, temperature=t, repetition_penalty=r,
                                             early_stop_num=40, rng_keys=[keys[b]])
        assert idxs[b] == ia[0] and ys[b].tolist() == ya[0].tolist(), f"row {b} keyed {keys[b]} draws differently in the session"


# ---- 3. admission, fp16 engine ----

@pytest.fixture(scope="module")
def forced48(v2):
    """48 rows, the fp32 engine's greedy ids with EOS forced at a hash-chosen step in 8 .. 40, and the fp32 logits of that
    teacher-forced decode"""
    from gsv import synthetic as S
    cfg, sd = v2
    N, cap = 48, 40
    EOS = cfg["model"]["vocab_size"] - 1
    xs, berts, prompts = _rows(cfg, N, seed=48, zh_bert=True)
    xd, bd = _dev(xs, berts)
    pd = [p.to(DEV) for p in prompts]
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, early_stop_num=cap, repetition_penalty=1.35)
    e32 = _engine(cfg, sd, torch.float32, max_batch=64, max_seq=320)
    y, i = e32.infer_panel_batch_infer(xd, None, pd, bd, **kw)
    assert i == [cap] * N
    ends = (S.hash_ints("ses_end", N, 33, 0) + 8).tolist()
    force = torch.full((N, cap + 1), EOS, dtype=torch.int32)
    for b in range(N):
        force[b, :ends[b]] = y[b][pd[b].numel():pd[b].numel() + ends[b]].to(torch.int32).cpu()
    y, i = e32.infer_panel_batch_infer(xd, None, pd, bd, force_tokens=force, dump_logits=True, **kw)
    assert i == ends and min(ends) >= 8 and max(ends) <= 40 and len(set(ends)) > 8
    L32 = e32.last_logits_dump.cpu().numpy()
    del e32
    torch.cuda.empty_cache()
    return xd, bd, pd, prompts, kw, force, ends, L32


@pytest.mark.parametrize("slots", [32, 36])
def test_fp16_engine_admission_teacher_forced_vs_fp32(v2_f16, forced48, slots):
    eng = v2_f16
    xd, bd, pd, prompts, kw, force, ends, L32 = forced48
    N = len(xd)
    ys, idxs = eng.infer_panel_continuous(xd, pd, bd, rng_keys=[(0, b) for b in range(N)], slots=slots, chunk=8, admit_min=4,
                                          force_tokens=force, dump_logits=True, **kw)
    ses = eng.last_session
    assert ses.modes and set(ses.modes) == {1}, "every advance must run on the persistent engine"
    assert eng.engine_stats()[1] == 0
    use = _slot_use(eng)
    assert sum(use.values()) == N and max(use.values()) >= 2, "slots must be reused"
    assert idxs == ends
    worst = 0.0
    for b in range(N):
        assert ys[b].cpu().tolist() == prompts[b].tolist() + force[b, :ends[b]].tolist()
        L16 = eng.last_logits_dump[b].cpu().numpy()
        assert L16.shape == (ends[b] + 1, L32.shape[2]) and np.isfinite(L16).all()
        err = np.abs(L16 - L32[:ends[b] + 1, b]).max(1)
        worst = max(worst, float(err.max()))
        assert err.max() <= 5e-2, f"row {b}: engine logits leave the 5e-2 band at step {err.argmax()} ({err.max():.3e})"
    print(f"[session] {slots} slots, {N} rows: teacher-forced fp16 engine vs fp32 max {worst:.3e}, "
          f"{len(ses.adopt)} admissions, {len(ses.modes)} advances")


# ---- 4. untouched neighbours ----

def _kv_of(eng, row, n_pos):
    last = eng.num_layers - 1
    return [eng.debug_kv(layer, which, row, n_pos).clone() for layer in (0, last) for which in (0, 1)]


@pytest.mark.parametrize("which", ["fp32", "fp16"])
def test_an_admission_leaves_its_neighbours_untouched(small, v2, v2_f16, which):
    cfg, eng = (small[0], small[2]) if which == "fp32" else (v2[0], v2_f16)
    xs, berts, prompts = _rows(cfg, 6, seed=61, zh_bert=True)
    xd, bd = _dev(xs, berts)
    pd = [p.to(DEV) for p in prompts]
    rows = _session_rows(xd, bd, pd, [(9, b) for b in range(6)])
    kw = dict(top_k=15, top_p=1.0, temperature=1.0, early_stop_num=40, repetition_penalty=1.35)
    with eng.open_session(6, **kw) as ses:
        ses.admit(rows[:3], slots=[0, 2, 5])
        assert ses.advance(4) == []
        st0 = ses.state()
        assert st0[1].tolist() == [1, 0, 1, 0, 0, 1] and st0[2].tolist() == [5, 0, 5, 0, 0, 5]
        n_pos = {s: int(st0[0][s]) + 8 for s in (0, 2, 5)}          # beyond what is cached: nothing may land there either
        kv0 = {s: _kv_of(eng, s, n_pos[s]) for s in (0, 2, 5)}
        ses.admit(rows[3:5], slots=[3, 1])
        st1 = ses.state()
        for s in (0, 2, 5):
            assert all(torch.equal(a, b) for a, b in zip(kv0[s], _kv_of(eng, s, n_pos[s]))), f"slot {s}: K/V changed"
            assert st1[:, s].tolist() == st0[:, s].tolist(), f"slot {s}: row state changed"
        assert st1[1].tolist() == [1, 1, 1, 1, 0, 1] and st1[2].tolist() == [5, 1, 5, 1, 0, 5]
        assert st1[3, 3] == pd[3].numel() and st1[0, 1] == xd[4].numel() + pd[4].numel()
        # refused admissions: a live slot, a repeated slot, a row that does not fit max_seq -- nothing changes
        kv1 = {s: _kv_of(eng, s, int(st1[0][s])) for s in (1, 3)}
        long_row = dict(rows[5], x=torch.zeros(eng.max_seq, dtype=torch.long, device=DEV), bert=None)
        for bad_rows, bad_slots in (([rows[5]], [2]), ([rows[5], rows[5]], [4, 4]), ([long_row], [4])):
            with pytest.raises(RuntimeError, match=r"rc=-1"):
                ses.admit(bad_rows, slots=bad_slots)
            st2 = ses.state()
            assert np.array_equal(st2, st1) and ses.free == [4]
            for s in (1, 3):
                assert all(torch.equal(a, b) for a, b in zip(kv1[s], _kv_of(eng, s, int(st1[0][s]))))
        ses.admit([rows[5]], slots=[4])            # the session goes on as if nothing had been refused
        done = []
        while ses.live:
            done += ses.advance(16)
        assert sorted(t for t, _, _ in done) == list(range(6))


# ---- 5. lifecycle ----

def test_the_ordinary_path_is_closed_during_a_session_and_unchanged_after(small):
    cfg, sd, eng = small
    xs, berts, prompts = _rows(cfg, 5, seed=3, zh_bert=True)
    xd, bd = _dev(xs, berts)
    pd = [p.to(DEV) for p in prompts]
    kw = dict(top_k=15, top_p=1.0, temperature=1.0, early_stop_num=20, repetition_penalty=1.35)
    before = eng.infer_panel_batch_infer(xd, None, pd, bd, seed=5, **kw)
    with eng.open_session(4, **kw) as ses:
        ses.admit(_session_rows(xd[:2], bd[:2], pd[:2], [(1, 0), (1, 1)]))
        with pytest.raises(RuntimeError, match=r"rc=-3"):
            eng.infer_panel_batch_infer(xd, None, pd, bd, seed=5, **kw)
        with pytest.raises(RuntimeError, match=r"rc=-3"):
            eng.open_session(4, **kw)
        assert ses.state()[1].tolist() == [1, 1, 0, 0], "the refused calls changed nothing"
        ses.advance(3)
    after = eng.infer_panel_batch_infer(xd, None, pd, bd, seed=5, **kw)
    assert before[1] == after[1] and [y.tolist() for y in before[0]] == [y.tolist() for y in after[0]]
