"""GPU: the AR prefill's K/V fill and attention alone (gsv_op_prefill_attn over the engine's own routing code) against the
float64 mirror of tests/_attnref.py, element by element, on every side of the flash kernel's edges.

fp16: route 1 (fused K/V + V^T launch, MFMA flash kernel), route 2 (split scatter + V^T, flash kernel), route 3 (scatter +
scalar kernel); fp32: route 3; route 0 is the engine's default and must equal route 1 (fp16) / route 3 (fp32) bit for bit.
Bars per element: flash 2^-11 |ref| + 2^-11 A + S 2^-25; scalar fp16 2^-11 |ref| + 2e-5; scalar fp32 2e-5.

Every case asserts: all of `out` within the route's bar in the flat, sharp and adversarial regimes; the cache rows j < S_b
bit-equal to the K / V columns of qkv; NaN sentinels intact behind every cache row's S_b and in 64 guard rows of `out`
(which also shows that no route reads a key beyond S_b: a NaN key or value would poison the output); every out row finite;
a second launch bit-identical; routes 1 and 2 bit-identical in out and both caches.  The ragged batch and its reverse give,
row by row, the bits of the row launched alone.  One engine-level test covers what the op cannot: the V^T scratch that grows
on demand and is shared by layers and batches."""
import ctypes as C
import functools
import os

import pytest
import torch

import _attnref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
CONFIGS = [(torch.float16, 1), (torch.float16, 2), (torch.float16, 3), (torch.float32, 3)]
ROUTE_NAME = {(torch.float16, 1): "flash fused (1)", (torch.float16, 2): "flash split (2)", (torch.float16, 3): "scalar fp16 (3)",
              (torch.float32, 3): "scalar fp32 (3)"}
WORST = {}      # (route name, regime) -> worst err / bar over the cases run so far
_RESULTS = {}   # launches already checked: (rows, H, regime, dtype, route) -> (out, kc, vc) on the host


def _ints(v):
    return (C.c_int32 * len(v))(*v)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


@functools.lru_cache(maxsize=None)
def _inputs(rows, H, regime, dtype):
    """the packed inputs and their mirror, computed once per (rows, H, regime, dtype) and shared by the routes"""
    xl, pl = [x for x, _ in rows], [p for _, p in rows]
    qkv = R.make_qkv(xl, pl, H, regime, dtype)
    ref, A = R.prefill_attn_ref(qkv, xl, pl, H)
    return qkv, ref, A


def _op(qkv_d, rows, H, dtype, route):
    """one call on NaN-filled outputs -> rc, (out with guard rows, kc, vc) on the host"""
    from gsv import _lib
    _lib.init(0)
    xl, pl = [x for x, _ in rows], [p for _, p in rows]
    B, d, M = len(rows), R.HD * H, sum(xl) + sum(pl)
    smax = max(x + p for x, p in rows) + 2          # the tightest arena the op accepts
    nan = float("nan")
    kc = torch.full((B, H, smax, R.HD), nan, dtype=dtype, device=DEV)
    vc = torch.full((B, H, smax, R.HD), nan, dtype=dtype, device=DEV)
    out = torch.full((M + GUARD, d), nan, dtype=dtype, device=DEV)
    torch.cuda.synchronize()
    rc = _lib.lib().gsv_op_prefill_attn(qkv_d.data_ptr(), _ints(xl), _ints(pl), B, H, d, smax, _lib.dtype_code(dtype), route,
                                        kc.data_ptr(), vc.data_ptr(), out.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, (out.cpu(), kc.cpu(), vc.cpu())


def _launch(rows, H, regime, dtype, route):
    """assertions 1-4 of the module docstring for one (rows, regime, dtype, route); the checked result is kept"""
    from gsv import _lib
    key = (rows, H, regime, dtype, route)
    if key in _RESULTS:
        return _RESULTS[key]
    what = f"{ROUTE_NAME.get((dtype, route), route)} {regime} rows={list(rows)} H={H}"
    qkv, ref, A = _inputs(rows, H, regime, dtype)
    xl, pl = [x for x, _ in rows], [p for _, p in rows]
    off, M = R.row_offsets(xl, pl)
    d = R.HD * H
    qkv_d = qkv.to(DEV)
    rc, (out, kc, vc) = _op(qkv_d, rows, H, dtype, route)
    _lib.check(rc, what)
    # sentinels and finiteness
    assert torch.isnan(out[M:]).all(), f"{what}: guard rows behind out were written"
    assert torch.isfinite(out[:M]).all(), f"{what}: non-finite output rows"
    for b, (X, P) in enumerate(rows):
        S = X + P
        assert torch.isnan(kc[b, :, S:]).all() and torch.isnan(vc[b, :, S:]).all(), f"{what}: cache of row {b} written at j >= S"
        # cache rows = the K / V columns of the packed qkv, bit for bit
        blk = qkv[off[b]:off[b] + S]
        k = blk[:, d:2 * d].reshape(S, H, R.HD).transpose(0, 1)
        v = blk[:, 2 * d:].reshape(S, H, R.HD).transpose(0, 1)
        assert torch.equal(_bits(kc[b, :, :S]), _bits(k)), f"{what}: K cache of row {b}"
        assert torch.equal(_bits(vc[b, :, :S]), _bits(v)), f"{what}: V cache of row {b}"
    # every element against the mirror
    if route != 0:
        worst = R.check(out[:M], ref, R.route_bar(route, dtype, ref, A, xl, pl), what)
        k2 = (ROUTE_NAME[(dtype, route)], regime)
        WORST[k2] = max(WORST.get(k2, 0.0), worst)
        print(f"[prefill_attn] {what}: worst err/bar {worst:.3f}")
    # a second launch gives the same bits
    rc, (out2, kc2, vc2) = _op(qkv_d, rows, H, dtype, route)
    _lib.check(rc, what)
    assert torch.equal(_bits(out2[:M]), _bits(out[:M])) and torch.isnan(out2[M:]).all(), f"{what}: second launch differs"
    for b, (X, P) in enumerate(rows):
        S = X + P
        assert torch.equal(_bits(kc2[b, :, :S]), _bits(kc[b, :, :S])) and torch.equal(_bits(vc2[b, :, :S]), _bits(vc[b, :, :S]))
    _RESULTS[key] = (out, kc, vc)
    return _RESULTS[key]


def _same_bits(a, b, rows, what):
    M = sum(x + p for x, p in rows)
    assert torch.equal(_bits(a[0][:M]), _bits(b[0][:M])), f"{what}: out differs"
    for i, (X, P) in enumerate(rows):
        assert torch.equal(_bits(a[1][i, :, :X + P]), _bits(b[1][i, :, :X + P])), f"{what}: K cache differs"
        assert torch.equal(_bits(a[2][i, :, :X + P]), _bits(b[2][i, :, :X + P])), f"{what}: V cache differs"


def _switch_set():
    return "GSV_SCALAR_PREFILL_ATTN" in os.environ or "GSV_PREFILL_SPLIT_SCATTER" in os.environ


def _case(rows, H):
    for regime in R.REGIMES:
        if regime == "adversarial":
            qkv = _inputs(rows, H, regime, torch.float16)[0]
            xl, pl = [x for x, _ in rows], [p for _, p in rows]
            if sum(pl) > 0:   # a bad input, not a kernel failure: pick another seed in _attnref.make_qkv
                assert R.hidden_mass_fraction(qkv, xl, pl, H) >= 0.9, "adversarial input does not load the hidden keys"
        res = {(dt, rt): _launch(rows, H, regime, dt, rt) for dt, rt in CONFIGS}
        _same_bits(res[(torch.float16, 1)], res[(torch.float16, 2)], rows, f"routes 1 and 2, {regime}")
        for dt, same in ((torch.float16, 1), (torch.float32, 3)):
            r0 = _launch(rows, H, regime, dt, 0)
            if not _switch_set():
                _same_bits(r0, res[(dt, same)], rows, f"route 0 and route {same}, {regime}, {dt}")


@pytest.mark.parametrize("X,P", R.SHAPES, ids=[f"X{x}_P{p}" for x, p in R.SHAPES])
def test_single_row(X, P):
    _case(((X, P),), 2)


def test_four_heads():
    _case(((37, 50),), 4)


def test_ragged_batch_rows_equal_the_rows_alone():
    """the batch in both orders: every assertion of a single case, and each row's out and caches bit-identical to the same row
    launched alone and to the same row of the reversed batch (tiling depends on (q0, X, S) of the row only; maxS changes
    strides, not arithmetic)"""
    fwd, rev = tuple(R.RAGGED), tuple(reversed(R.RAGGED))
    _case(fwd, 2)
    _case(rev, 2)
    n = len(fwd)
    off_f, _ = R.row_offsets([x for x, _ in fwd], [p for _, p in fwd])
    off_r, _ = R.row_offsets([x for x, _ in rev], [p for _, p in rev])
    for regime in R.REGIMES:
        for dt, rt in CONFIGS:
            f, r = _launch(fwd, 2, regime, dt, rt), _launch(rev, 2, regime, dt, rt)
            for b, (X, P) in enumerate(fwd):
                S, what = X + P, f"{ROUTE_NAME[(dt, rt)]} {regime} row {b} {(X, P)}"
                alone = _launch(((X, P),), 2, regime, dt, rt)
                rb = n - 1 - b
                for name, got in (("batch", (f[0][off_f[b]:off_f[b] + S], f[1][b, :, :S], f[2][b, :, :S])),
                                  ("reversed batch", (r[0][off_r[rb]:off_r[rb] + S], r[1][rb, :, :S], r[2][rb, :, :S]))):
                    assert torch.equal(_bits(got[0]), _bits(alone[0][:S])), f"{what}: out in the {name} differs from the row alone"
                    assert torch.equal(_bits(got[1]), _bits(alone[1][0, :, :S])), f"{what}: K cache in the {name}"
                    assert torch.equal(_bits(got[2]), _bits(alone[2][0, :, :S])), f"{what}: V cache in the {name}"


@pytest.mark.parametrize("case", R.REFUSALS, ids=[c[0] for c in R.REFUSALS])
def test_refusals_leave_the_outputs_untouched(case):
    from gsv import _lib
    _lib.init(0)
    _, present, xl, pl, H, d, smax, code, route, msg = case
    dtype = torch.float16 if code == 1 else torch.float32
    nan = float("nan")
    qkv = torch.zeros(64, 3 * d, dtype=dtype, device=DEV)
    kc = torch.full((len(xl), H, smax, d // H), nan, dtype=dtype, device=DEV)
    vc = torch.full_like(kc, nan)
    out = torch.full((64 + GUARD, d), nan, dtype=dtype, device=DEV)
    torch.cuda.synchronize()
    ptr = [t.data_ptr() if p else None for t, p in zip((qkv, kc, vc, out), present)]
    rc = _lib.lib().gsv_op_prefill_attn(ptr[0], _ints(xl), _ints(pl), len(xl), H, d, smax, code, route, ptr[1], ptr[2], ptr[3], None)
    torch.cuda.synchronize()
    assert rc != 0
    assert msg in _lib.lib().gsv_last_error().decode()
    assert torch.isnan(kc).all() and torch.isnan(vc).all() and torch.isnan(out).all()


def test_vt_scratch_grows_and_is_reused_across_batches():
    """The V^T scratch is allocated on demand (t2s_prefill_rows) and shared by all layers and rows: a short batch, a long one
    that makes it grow, and the short one again on ONE fp16 engine each give the ids and per-step logits, bit for bit, of a
    fresh engine that decodes that batch alone (stale columns of a longer batch, or a stride left over from it, would show)."""
    from gsv import synthetic as S
    from gsv.AR.models.t2s_model import Text2SemanticDecoder
    from oracle import cases
    cfg, sd, *_ = cases.t2s_case_inputs(cases.T2S_CASES["t2s_small_greedy"])
    m = cfg["model"]

    def engine():
        e = Text2SemanticDecoder(cfg, device=DEV, dtype=torch.float16, max_batch=8, max_seq=320)
        e.load_state_dict(sd)
        return e

    def batch(tag, shapes):
        xs = [torch.from_numpy(S.hash_ints(f"vt_x_{tag}{i}", x, m["phoneme_vocab_size"], 3)).long().to(DEV) for i, (x, _) in enumerate(shapes)]
        berts = [S.hash_symmetric(f"vt_b_{tag}{i}", (1024, x), 0.5, 3).to(DEV) for i, (x, _) in enumerate(shapes)]
        prompts = [torch.from_numpy(S.hash_ints(f"vt_p_{tag}{i}", p, m["vocab_size"] - 1, 3)).long().to(DEV) for i, (_, p) in enumerate(shapes)]
        return xs, berts, prompts

    short = batch("s", [(17, 23), (9, 30)])                                            # S = 40, 39
    long_ = batch("l", [(37, 50), (40, 260), (6, 1), (5, 290), (33, 64), (38, 200)])   # S up to 300
    kw = dict(top_k=1, top_p=1.0, temperature=1.0, early_stop_num=8, repetition_penalty=1.35, dump_logits=True)

    def decode(eng, b):
        xs, berts, prompts = b
        ys, idx = eng.infer_panel_batch_infer(xs, None, prompts, berts, **kw)
        return [y.cpu().tolist() for y in ys], idx, eng.last_logits_dump.cpu()

    want_short, want_long = decode(engine(), short), decode(engine(), long_)
    eng = engine()
    for name, b, want in (("short", short, want_short), ("long", long_, want_long), ("short again", short, want_short)):
        ys, idx, logits = decode(eng, b)
        assert torch.isfinite(logits).all()
        assert (ys, idx) == want[:2], f"{name}: ids differ from a fresh engine's"
        assert torch.equal(logits, want[2]), f"{name}: logits differ from a fresh engine's"


def test_zz_worst_err_over_bar_table():
    """prints what the cases above measured (the figures DESIGN.md quotes); the bars themselves are asserted per case"""
    for name in ROUTE_NAME.values():
        print(f"[prefill_attn] worst err/bar, {name}: " +
              ", ".join(f"{rg} {WORST[(name, rg)]:.3f}" for rg in R.REGIMES if (name, rg) in WORST))
    assert all(v <= 1.0 for v in WORST.values())
