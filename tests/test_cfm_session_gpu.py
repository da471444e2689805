"""GPU: flow-matching sessions (gsv_cfm_session_*, CFM.open_session): rows with their own step count, guidance rate, prompt
and LoRA slot that enter and leave one pass between Euler steps.  Every row is held to the oracle run on that row alone
(oracle/cfm_oracle.py unguided, tests/_cfg_ref.py guided) with its own n_steps and rate; a session whose rows share one setting
is held, bit for bit, to the one-shot pass whose kernels the per-row forms mirror."""
import ctypes as C
import functools

import pytest
import torch

import _cfg_ref
from _parity import dit_v3_chunk_case
from gsv import synthetic as S
from oracle import cfm_oracle
from test_cfm_rows_gpu import DEV, _cfm, _check_fp16_row, _rows, _small

pytestmark = pytest.mark.gpu
T = 40
#           n_steps, rate, Tp
ROWS = ((2, 0.0, 0), (3, 0.0, 17), (4, 0.7, 1), (3, 2.0, T - 1), (5, 0.0, T), (1, 0.7, 9))
CAP = 6


def _inputs():
    cfg, sd, t, _, _ = _small()
    assert t == T
    mu, prompts, noise = _rows(cfg, T, [r[2] for r in ROWS], "sess")
    return cfg, sd, mu, prompts, noise


def _oracle(sd, cfg, mu, prompt, steps, noise, rate):
    if rate > 1e-5:
        return _cfg_ref.cfm_inference_cfg(sd, cfg, mu, prompt, steps, noise.clone(), rate)
    return cfm_oracle.cfm_inference(sd, cfg, mu, prompt, steps, noise.clone())


@functools.lru_cache(maxsize=None)
def _refs():
    """every row through the oracle alone, with its own step count and rate; once per test session"""
    cfg, sd, mu, prompts, noise = _inputs()
    return tuple(_oracle(sd, cfg, mu[b:b + 1], prompts[b], n, noise[b:b + 1], r) for b, (n, r, _) in enumerate(ROWS))


def _admit(sess, rows, inputs, **kw):
    _, _, mu, prompts, noise = inputs
    return sess.admit(mu[rows].to(DEV), [prompts[b].to(DEV) for b in rows], [ROWS[b][0] for b in rows], [ROWS[b][1] for b in rows],
                      noise=noise[rows], **kw)


def _staggered(cfm, release_row=None):
    """The schedule of the file: rows 0-2, a step, rows 3-4 refused (7 DiT rows > 6), a step, row 0 fetched, rows 3-4 admitted
    (row 3 into row 0's slot), a step, row 1 fetched, row 5 refused (a guided row, one free DiT row), a step, row 2 fetched,
    row 5 into row 1's slot, steps to the end.  -> ({row: mel [1, mel, T]}, the events seen)"""
    inputs = _inputs()
    out, ev = {}, []
    with cfm.open_session(CAP, T) as sess:
        slot = dict(zip((0, 1, 2), _admit(sess, [0, 1, 2], inputs)))
        assert slot == {0: 0, 1: 1, 2: 2}
        assert sess.step(1) == []
        with pytest.raises(RuntimeError, match="exceed rows_cap"):
            _admit(sess, [3, 4], inputs)
        ev.append("refused")
        assert sess.step(1) == [slot[0]]
        assert sess.state[slot[0]] == (sess.FINISHED, 2, 2) and sess.state[slot[1]] == (sess.LIVE, 2, 3)
        out[0] = sess.fetch(slot[0])
        assert sess.state[slot[0]][0] == sess.FREE
        slot.update(zip((3, 4), _admit(sess, [3, 4], inputs)))
        assert slot[3] == slot[0] and slot[4] == 3
        ev.append("refill")
        if release_row is not None:
            sess.release([slot[release_row]])
            assert sess.state[slot[release_row]] == (sess.FREE, 0, 0)
        assert sess.step(1) == [slot[1]]
        out[1] = sess.fetch(slot[1])
        if release_row is None:
            with pytest.raises(RuntimeError, match="exceed rows_cap"):       # live: rows 2, 3 (guided) and 4 = 5 DiT rows
                _admit(sess, [5], inputs)
            ev.append("refused guided")
        assert sess.step(1) == [slot[2]]
        out[2] = sess.fetch(slot[2])
        slot[5] = _admit(sess, [5], inputs)[0]
        assert slot[5] == (slot[1] if release_row is None else slot[release_row])      # the lowest free slot
        done = sess.step(1)
        assert done == sorted(slot[r] for r in (3, 5) if r != release_row)
        for r in (3, 5):
            if r != release_row:
                out[r] = sess.fetch(slot[r])
        assert sess.step(5) == [slot[4]]                                     # two steps run, then no row is live
        assert sess.state[slot[4]] == (sess.FINISHED, 5, 5)
        out[4] = sess.fetch(slot[4])
        assert all(st == (sess.FREE, 0, 0) for st in sess.state)
    return {r: o.float().cpu()[None] for r, o in out.items()}, ev


def _check_fp32_row(o, ref, Tp, label):
    err = (o - ref).abs().max().item()
    print(f"[parity] {label}: max-abs error {err:.2e}")
    assert torch.isfinite(o).all() and err <= 2e-3
    assert Tp == 0 or float(o[..., :Tp].abs().max()) == 0.0


def test_fp32_staggered_session_matches_the_oracle_row_by_row():
    """fp32: six rows with their own (n_steps, rate, Tp), admitted at three different times into a session of 6 DiT rows, with
    a refusal, a fetch and a refill into the freed slot.  Each row within the fp32 CFM bar (2e-3 max-abs, test_cfm_gpu.py) of
    the oracle run on it alone; prompt frames exactly 0; the Tp = T row all zeros."""
    cfg, sd, _, _, _ = _inputs()
    out, ev = _staggered(_cfm(cfg, sd, torch.float32))
    assert ev == ["refused", "refill", "refused guided"] and sorted(out) == list(range(6))
    for b, ref in enumerate(_refs()):
        _check_fp32_row(out[b], ref, ROWS[b][2], f"fp32 session row {b} {ROWS[b]}")
    assert float(out[4].abs().max()) == 0.0 and float(out[3][..., -1].abs().max()) > 0.0


def test_fp16_staggered_session_matches_the_oracle_row_by_row():
    """the same schedule through the fp16 engine: the fp16 DiT bar of test_cfm_rows_gpu.py (_check_fp16_row)"""
    cfg, sd, _, _, _ = _inputs()
    out, _ = _staggered(_cfm(cfg, sd, torch.float16))
    for b, ref in enumerate(_refs()):
        _check_fp16_row(out[b], ref, ROWS[b][2], f"fp16 session row {b} {ROWS[b]}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("case", ["unguided", "guided", "lora"])
def test_uniform_session_is_the_one_shot_pass_bit_for_bit(dtype, case):
    """B = 4 rows admitted together with n_steps = 3: step(3) is torch.equal to inference_rows, and three step(1) to step(3).
    Unguided, rate 0.7 (the twins packed behind the rows, as the one-shot pass packs them), and LoRA slots [0, None, 1, 0]."""
    from test_cfm_lora_gpu import _engine
    cfg, sd, _, _, _ = _inputs()
    B, steps = 4, 3
    mu, prompts, noise = _rows(cfg, T, [0, 17, 1, T - 1], "uniform")
    cfm = _engine(dtype) if case == "lora" else _cfm(cfg, sd, dtype)
    rate = 0.7 if case == "guided" else 0.0
    adapters = [0, None, 1, 0] if case == "lora" else None
    dev = [p.to(DEV) for p in prompts]
    want = cfm.inference_rows(mu.to(DEV), dev, steps, noise=noise, inference_cfg_rate=rate, adapters=adapters)

    def run(ks):
        with cfm.open_session(2 * B if rate else B, T) as sess:
            slots = sess.admit(mu.to(DEV), dev, steps, rate, noise=noise, adapters=adapters)
            assert slots == list(range(B))
            for i, k in enumerate(ks):
                assert sess.step(k) == (slots if i == len(ks) - 1 else [])
            return torch.stack([sess.fetch(s) for s in slots])
    once = run([3])
    assert torch.isfinite(once).all() and float(once.abs().max()) > 0
    assert torch.equal(once, want.float())
    assert torch.equal(run([1, 1, 1]), once)
    # the sequence form of inference_rows serves the same rows through a session of its own
    assert torch.equal(cfm.inference_rows(mu.to(DEV), dev, [steps] * B, noise=noise, inference_cfg_rate=[rate] * B, adapters=adapters), want)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_sessions_repeat_and_rows_do_not_see_their_neighbours(dtype):
    """the staggered schedule replayed gives identical bits; in a session of 5 rows with equal n_steps, swapping the prompts of
    two rows changes those two rows and no other, bit for bit"""
    cfg, sd, _, _, _ = _inputs()
    cfm = _cfm(cfg, sd, dtype)
    a, _ = _staggered(cfm)
    b, _ = _staggered(cfm)
    assert all(torch.equal(a[r], b[r]) for r in range(6))
    _, _, _, tps, steps = _small()
    mu, prompts, noise = _rows(cfg, T, tps, "rows")
    dev = [p.to(DEV) for p in prompts]

    def run(ps):
        with cfm.open_session(5, T) as sess:
            slots = sess.admit(mu.to(DEV), ps, steps, 0.0, noise=noise)
            assert sess.step(steps) == slots
            return [sess.fetch(s) for s in slots]
    x = run(dev)
    sw = list(dev)
    sw[1], sw[2] = dev[2], dev[1]
    y = run(sw)
    for r in (0, 3, 4):
        assert torch.equal(x[r], y[r]), f"row {r} changed with the prompts of rows 1 and 2"
    assert not torch.equal(x[1], y[1]) and not torch.equal(x[2], y[2])


def test_releasing_a_live_row_leaves_the_others_at_their_oracle():
    """fp32: row 3 (guided, live, one step taken by nobody yet) is released right after its admission; `state` reports its slot
    free, and every other row stays within the fp32 bar of its oracle"""
    cfg, sd, _, _, _ = _inputs()
    out, _ = _staggered(_cfm(cfg, sd, torch.float32), release_row=3)
    assert sorted(out) == [0, 1, 2, 4, 5]
    for b, ref in enumerate(_refs()):
        if b != 3:
            _check_fp32_row(out[b], ref, ROWS[b][2], f"fp32 session with row 3 released, row {b}")


def _raw_admit(cfm, slots, mu, ptrs, tps, steps, rates, noise):
    from gsv import _lib
    n = len(slots)
    dit = cfm.estimator
    rc = _lib.lib().gsv_cfm_session_admit(dit._h, n, (C.c_int32 * n)(*slots), mu.data_ptr(), (C.c_void_p * n)(*ptrs), (C.c_int * n)(*tps),
                                          None, (C.c_int * n)(*steps), (C.c_float * n)(*rates), noise.data_ptr(), None,
                                          C.c_void_p(dit.stream.cuda_stream))
    dit.stream.synchronize()
    return rc


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_refused_calls_return_an_error_and_write_nothing(dtype):
    """admission into an occupied slot or past the cap, n_steps 0 / 1025, Tp > T, a null prompt with Tp > 0, fetch of a live
    slot, a one-shot entry while the session is open, begin twice: each returns an error; the NaN sentinels of every output
    buffer stay intact and the session's rows come out with the bits of an undisturbed session"""
    from gsv import _lib
    cfg, sd, _, _, _ = _inputs()
    cfm = _cfm(cfg, sd, dtype)
    dit, lib, md = cfm.estimator, _lib.lib(), cfg["mel_dim"]
    mu, prompts, noise = _rows(cfg, T, [5, 9, 0], "refuse")
    stream = C.c_void_p(dit.stream.cuda_stream)

    def clean():
        with cfm.open_session(3, T) as sess:
            slots = sess.admit(mu[:2].to(DEV), [p.to(DEV) for p in prompts[:2]], [2, 3], 0.0, noise=noise[:2])
            sess.step(3)
            return [sess.fetch(s) for s in slots]
    want = clean()
    with torch.cuda.device(DEV):
        m, nz = mu.to(DEV).contiguous(), noise.to(DEV).contiguous()
        ps = [p.to(DEV).contiguous() for p in prompts]
        n, guard = md * T, 4096
        out = torch.full((3 * n + guard,), float("nan"), device=DEV)
        torch.cuda.synchronize()
        sess = cfm.open_session(3, T)
        assert lib.gsv_cfm_session_begin(dit._h, 3, T, 1.0, stream) != 0                                   # begin twice
        assert _raw_admit(cfm, [0, 1], m[:2], [ps[0].data_ptr(), ps[1].data_ptr()], [5, 9], [2, 3], [0.0, 0.0], nz[:2]) == 0
        one = (m[2:], [None], [0])
        assert _raw_admit(cfm, [1], *one, [2], [0.0], nz[2:]) != 0                                       # occupied slot
        assert _raw_admit(cfm, [3], *one, [2], [0.0], nz[2:]) != 0                                       # no such slot
        assert _raw_admit(cfm, [2], *one, [2], [0.7], nz[2:]) != 0                                       # past the cap: 2 + 2 DiT rows
        assert _raw_admit(cfm, [2], *one, [0], [0.0], nz[2:]) != 0 and _raw_admit(cfm, [2], *one, [1025], [0.0], nz[2:]) != 0
        assert _raw_admit(cfm, [2], m[2:], [ps[0].data_ptr()], [T + 1], [2], [0.0], nz[2:]) != 0        # Tp > T
        assert _raw_admit(cfm, [2], m[2:], [None], [4], [2], [0.0], nz[2:]) != 0                         # null prompt, Tp > 0
        assert lib.gsv_cfm_session_fetch(dit._h, 0, out.data_ptr(), stream) != 0                           # live slot
        assert lib.gsv_cfm_session_fetch(dit._h, 2, out.data_ptr(), stream) != 0                           # free slot
        tp1 = (C.c_int * 1)(0)
        assert lib.gsv_cfm_inference_rows(dit._h, m.data_ptr(), (C.c_void_p * 1)(None), tp1, 1, T, 2, nz.data_ptr(), None, 1.0,
                                          out.data_ptr(), stream) != 0                                     # one-shot entry, session open
        assert lib.gsv_cfm_inference(dit._h, m.data_ptr(), None, 1, T, 0, 2, nz.data_ptr(), 1.0, 0, out.data_ptr(), stream) != 0
        assert sess.state == [(sess.LIVE, 0, 2), (sess.LIVE, 0, 3), (sess.FREE, 0, 0)]
        torch.cuda.synchronize()
        assert torch.isnan(out).all()
        assert sess.step(3) == [0, 1]
        for s in (0, 1):
            sess.fetch(s, out[s * n:(s + 1) * n])
        torch.cuda.synchronize()
        assert torch.isnan(out[2 * n:]).all()
        for s in (0, 1):
            assert torch.equal(out[s * n:(s + 1) * n].view(md, T), want[s])
        sess.close()
        assert lib.gsv_cfm_session_step(dit._h, 1, stream) != 0                                            # no session
        again = cfm.inference_rows(mu[:2].to(DEV), ps[:2], 2, noise=noise[:2])                            # works again after end
        assert torch.isfinite(again).all()


def test_fp16_production_widths_two_gate_vectors_in_one_tile():
    """DiT 1024 x 22, T = 934, fp16.  Row 0 is the chunk case of tests/_parity.py (Tp = 468, 2 steps, oracle output included);
    row 1 is admitted after row 0's first step, without a prompt and with n_steps = 1, and is held to one oracle forward.  The
    second step runs the production GEMM routes at R = 2 x 934 rows with two different gate vectors (row 0 at step 1 of 2, row 1
    at step 0 of 1) inside one 64- / 128-row tile, right after the live set changed.  Both rows within the fp16 DiT bar."""
    cfg, sd, mu0, prompt0, noise0, steps, ref0 = dit_v3_chunk_case()
    assert steps == 2 and mu0.shape[1] == 934
    mu1, p1, nz1 = _rows(cfg, 934, [0], "sess1024")
    torch.set_num_threads(8)
    ref1 = cfm_oracle.cfm_inference(sd, cfg, mu1, p1[0], 1, nz1.clone())
    cfm = _cfm(cfg, sd, torch.float16)
    with cfm.open_session(2, 934) as sess:
        assert sess.admit(mu0.to(DEV), [prompt0.to(DEV)], 2, 0.0, noise=noise0) == [0]
        assert sess.step(1) == []
        assert sess.admit(mu1.to(DEV), [p1[0].to(DEV)], 1, 0.0, noise=nz1) == [1]
        assert sess.step(1) == [0, 1]
        o0, o1 = sess.fetch(0).float().cpu()[None], sess.fetch(1).float().cpu()[None]
    _check_fp16_row(o0, ref0, 468, "fp16 depth-22 DiT session, row 0 (Tp = 468, 2 steps)")
    _check_fp16_row(o1, ref1, 0, "fp16 depth-22 DiT session, row 1 (no prompt, 1 step)")


def test_modulation_cache_evicts_and_refuses():
    """fp32.  The handle caches at most 8 modulation tables.  Nine rows with nine different step counts, one after the other
    through a session of one DiT row: the ninth admission drops the least recently used table (2 steps); a row with 2 steps
    admitted afterwards recomputes it and gives the bits it gave the first time.  Nine different step counts live at once are
    refused, and the eight rows already live finish as if nothing had been asked."""
    cfg, sd, _, _, _ = _inputs()
    cfm = _cfm(cfg, sd, torch.float32)
    mu, prompts, noise = _rows(cfg, T, [3] * 9, "cache")
    dev = [p.to(DEV) for p in prompts]

    def one(sess, b, n):
        slot = sess.admit(mu[b:b + 1].to(DEV), dev[b:b + 1], n, 0.0, noise=noise[b:b + 1])[0]
        assert sess.step(n) == [slot]
        return sess.fetch(slot)
    with cfm.open_session(1, T) as sess:
        first = [one(sess, 0, n) for n in range(2, 11)]          # 9 step counts: 2 .. 10
        again = one(sess, 0, 2)
    assert torch.equal(again, first[0]) and not torch.equal(first[1], first[0])
    with cfm.open_session(9, T) as sess:
        slots = sess.admit(mu[:8].to(DEV), dev[:8], list(range(2, 10)), 0.0, noise=noise[:8])
        with pytest.raises(RuntimeError, match="distinct step counts"):
            sess.admit(mu[8:].to(DEV), dev[8:], 11, 0.0, noise=noise[8:])
        assert sess.state[8] == (sess.FREE, 0, 0)
        assert sess.step(9) == slots
        got = sess.fetch(slots[0])
    assert torch.equal(got, first[0])


# ---- shapes at which the gated GEMMs (out-projection, FF2) take gemm_lds with per-row gates
WIDE_STEPS, WIDE_TPS = (1, 2, 2, 1, 1), (0, 468, 300, 0, 100)


@functools.lru_cache(maxsize=1)
def _wide_case():
    """DiT 1024 wide, 2 blocks deep, T = 934: five rows with their own step counts and prompts, each through the oracle alone"""
    cfg = dict(S.DIT_V3_CONFIG, depth=2)
    sd = S.make_dit_state_dict(cfg, seed=9)
    mu, prompts, noise = _rows(cfg, 934, list(WIDE_TPS), "sesswide")
    torch.set_num_threads(8)
    refs = tuple(cfm_oracle.cfm_inference(sd, cfg, mu[b:b + 1], prompts[b], n, noise[b:b + 1].clone()) for b, n in enumerate(WIDE_STEPS))
    return cfg, sd, mu, prompts, noise, refs


@pytest.mark.parametrize("B,waves", [(3, 8), (5, 4)], ids=["3rows_8wave", "5rows_4wave"])
def test_fp16_rows_at_different_steps_on_the_gemm_lds_route(B, waves):
    """fp16, D = 1024, T = 934.  B rows with n_steps 1 / 2 / 2 (/ 1 / 1) admitted together: at every step the rows stand at
    different steps of different step counts, so every 128-row tile that spans two utterances holds two gate vectors.  B = 3 is
    2802 rows (gemm_lds, 8 waves: the form that spills), B = 5 is 4670 rows (4 waves) in the first step and 1868 (gemm_t64)
    in the second.  The dispatcher's choice for the out-projection and FF2 at these shapes is read back through the op entry
    (family 4, flag 32 GROWS); every row within the fp16 DiT bar of the oracle run on it alone."""
    from test_gate_rows_gpu import dispatch_route
    cfg, sd, mu, prompts, noise, refs = _wide_case()
    inner, FF = cfg["heads"] * cfg["dim_head"], cfg["dim"] * cfg["ff_mult"]
    for K in (inner, FF):
        r = dispatch_route("f16", B * 934, K, cfg["dim"], 934)
        assert r[0] == 4 and r[2] == waves and r[7] & 32, f"K = {K}: {r}"
    cfm = _cfm(cfg, sd, torch.float16)
    with cfm.open_session(B, 934) as sess:
        slots = sess.admit(mu[:B].to(DEV), [p.to(DEV) for p in prompts[:B]], list(WIDE_STEPS[:B]), 0.0, noise=noise[:B])
        assert sess.step(1) == [s for s, n in zip(slots, WIDE_STEPS) if n == 1]
        assert sess.step(1) == [s for s, n in zip(slots, WIDE_STEPS) if n == 2]
        out = [sess.fetch(s).float().cpu()[None] for s in slots]
    for b in range(B):
        _check_fp16_row(out[b], refs[b], WIDE_TPS[b], f"fp16 D = 1024 session of {B} rows, row {b} ({WIDE_STEPS[b]} steps, Tp = {WIDE_TPS[b]})")


def test_fp32_thirteen_rows_on_the_gemm_lds_route():
    """fp32, small DiT, T = 40: 13 rows (520 rows >= 512, Cout = 128 >= 96) with n_steps 2 / 3 / 4 in turn take gemm_lds<fp32> with
    per-row gates in their first two steps (13 gate vectors, a boundary inside every 128-row tile); each row within the fp32 bar
    of the oracle run on it alone"""
    from test_gate_rows_gpu import dispatch_route
    cfg, sd, _, _, _ = _inputs()
    B = 13
    steps = [2 + b % 3 for b in range(B)]
    tps = [(7 * b) % 23 for b in range(B)]
    mu, prompts, noise = _rows(cfg, T, tps, "sess13")
    for K in (cfg["heads"] * cfg["dim_head"], cfg["dim"] * cfg["ff_mult"]):
        r = dispatch_route("f32", B * T, K, cfg["dim"], T)
        assert r[0] == 4 and r[1] == 0 and r[7] & 32, f"K = {K}: {r}"
    cfm = _cfm(cfg, sd, torch.float32)
    with cfm.open_session(B, T) as sess:
        slots = sess.admit(mu.to(DEV), [p.to(DEV) for p in prompts], steps, 0.0, noise=noise)
        done = sess.step(2) + sess.step(1) + sess.step(1)
        assert sorted(done) == slots
        out = [sess.fetch(s).float().cpu()[None] for s in slots]
    for b in range(B):
        ref = cfm_oracle.cfm_inference(sd, cfg, mu[b:b + 1], prompts[b], steps[b], noise[b:b + 1].clone())
        _check_fp32_row(out[b], ref, tps[b], f"fp32 session of 13 rows, row {b} ({steps[b]} steps)")


def test_release_after_a_step_repacks_the_live_rows():
    """fp32.  Rows 1, 2 (guided) and 3 (guided) are admitted and take one step, after which the packed input is up to date.
    Row 2 -- the middle slot, with a twin -- is released, and the next call steps with nothing but the release in between:
    the release alone must make the session repack (rows 1, 3 and one twin instead of rows 1, 2, 3 and two twins).  Rows 1 and
    3 stay within the fp32 bar of their oracle."""
    cfg, sd, _, _, _ = _inputs()
    inputs = _inputs()
    with _cfm(cfg, sd, torch.float32).open_session(5, T) as sess:
        slots = _admit(sess, [1, 2, 3], inputs)
        assert sess.step(1) == [] and [st[:2] for st in sess.state[:3]] == [(sess.LIVE, 1)] * 3
        sess.release([slots[1]])
        assert sess.state[slots[1]] == (sess.FREE, 0, 0)
        assert sess.step(2) == [slots[0], slots[2]]
        out = {1: sess.fetch(slots[0]).float().cpu()[None], 3: sess.fetch(slots[2]).float().cpu()[None]}
    for b in (1, 3):
        _check_fp32_row(out[b], _refs()[b], ROWS[b][2], f"fp32 session, row 2 released after a step, row {b}")


def test_an_adapter_in_use_by_a_live_row_cannot_be_removed():
    """remove_adapter of a slot that a live session row runs with is refused (the later steps would read freed weights); once
    the row is fetched the removal works"""
    from test_cfm_lora_gpu import _engine
    cfg, _, _, _, _ = _inputs()
    cfm = _engine(torch.float32)
    mu, prompts, noise = _rows(cfg, T, [0, 5], "sessad")
    with cfm.open_session(2, T) as sess:
        slots = sess.admit(mu.to(DEV), [p.to(DEV) for p in prompts], 2, 0.0, noise=noise, adapters=[0, None])
        sess.step(1)
        with pytest.raises(RuntimeError, match="live row"):
            cfm.remove_adapter(0)
        assert cfm.estimator.adapter_count() == 2
        cfm.remove_adapter(1)                                # no row uses slot 1
        assert sess.step(1) == slots
        a = sess.fetch(slots[0])
        assert torch.isfinite(a).all()
        cfm.remove_adapter(0)
    assert cfm.estimator.adapter_count() == 0
