"""GPU: flash_attn64_tile<QT> in its row and segmented launch forms and vt_kernel's rotary plane, through
gsv_op_flash_attn64_rows / gsv_op_flash_attn64_seg_qt, against the float64 mirror of tests/_attnmirror.py, element by element.

Every launch asserts: `out` and the V^T scratch arrive NaN-filled; every out element finite and inside the flash bar
2^-11 |ref| + 2^-11 A + T 2^-25 (with the NaN prefill: no query tile skipped by the XCD remap); the 64 guard rows behind `out`
and the 8 padding rows between utterances still NaN; a second launch on re-uploaded inputs bit-identical.  With the rotary, q and
k read back are inside the rotary bar, every other channel and V bit-unchanged, and the attention mirror is fed the device's
rotated bits.  QT is forced to 1, 2 and 4; the launcher's own rule is asserted through the route record."""
import functools

import pytest
import torch

import _attn_gpu as G
import _attnmirror as M

pytestmark = pytest.mark.gpu
F16 = torch.float16
W = G.Worst("attn_flash64")
_ALONE = {}


@functools.lru_cache(maxsize=None)
def _utt(T, H, regime, seed):
    return M.make_qkv(T, H, 64, regime, F16, seed=seed)


def _rows(T, H, regime, qt, seeds=(0,), rope_half=None):
    """one checked launch of the rows hook -> (out [rows][T][H 64], qkv read back [rows][T][3 H 64])"""
    from gsv import _lib
    what = f"rows T={T} H={H} rows={len(seeds)} qt={qt} rope={rope_half} {regime}"
    qkvs = [_utt(T, H, regime, s) for s in seeds]
    cs = M.rope_table(T, rope_half) if rope_half is not None else None
    rc, out, guard, back, vt = G.rows_call(qkvs, H, qt, cs, rope_half or 0)
    _lib.check(rc, what)
    fam, got_qt = G.last_route()
    assert fam == "rows" and (qt == 0 or got_qt == qt), f"{what}: the launch recorded {fam} QT {got_qt}"
    inner, ldv = H * 64, (T + 31) // 32 * 32
    assert torch.isnan(guard).all() and torch.isnan(out[:, T:]).all(), f"{what}: rows behind an utterance's out were written"
    assert torch.isnan(back[:, T:]).all(), f"{what}: the rotary wrote behind an utterance"
    assert torch.isfinite(vt[:, :inner * ldv]).all() and torch.isnan(vt[:, inner * ldv:]).all(), f"{what}: V^T scratch"
    for r, x in enumerate(qkvs):
        got = back[r, :T]
        if rope_half is None:
            assert torch.equal(G.bits(got), G.bits(x)), f"{what}: qkv of row {r} changed"
        else:
            ref, bar = M.rope_ref(x, cs, rope_half, H)
            W.add("rotary", regime, M.check(got, ref, bar, what + f" rotary row {r}"), what + f" rotary row {r}")
        ref, A = M.attn_ref(*M.split(got, H, 64), 0.125)
        W.add(f"rows QT{got_qt}", regime, M.check(out[r, :T], ref, M.flash_bar(ref, A, T), what + f" row {r}"), what + f" row {r}")
    rc, out2, guard2, back2, _ = G.rows_call(qkvs, H, qt, cs, rope_half or 0)
    _lib.check(rc, what)
    assert torch.equal(G.bits(out2[:, :T]), G.bits(out[:, :T])) and torch.equal(G.bits(back2[:, :T]), G.bits(back[:, :T])), \
        f"{what}: second launch differs"
    assert torch.isnan(guard2).all() and torch.isnan(out2[:, T:]).all()
    return out[:, :T], back[:, :T]


@pytest.mark.parametrize("T", M.ROWS_T)
def test_rows_every_qt(T):
    for regime in ("flat", "sharp"):
        for qt in (1, 2, 4):
            _rows(T, 2, regime, qt)


@pytest.mark.parametrize("T,H", M.ROWS_HEADS)
def test_rows_heads(T, H):
    for qt in (1, 2, 4):
        _rows(T, H, "sharp", qt)


@pytest.mark.parametrize("shape,want", M.ROWS_AUTO, ids=[f"T{t}_H{h}" for (t, h), _ in M.ROWS_AUTO])
def test_launcher_rule_picks_the_recorded_qt(shape, want):
    """qt = 0: the launcher's rule (cdiv(T, 64) heads and cdiv(T, 32) heads against 200), read from the route record; the
    existing gsv_op_flash_attn64 computes the same bits"""
    import os
    from gsv import _lib
    T, H = shape
    qkv = _utt(T, H, "sharp", 0)
    rc, out, guard, _, _ = G.rows_call([qkv], H, 0)
    _lib.check(rc, "rows hook")
    fam, qt = G.last_route()
    assert fam == "rows"
    if "GSV_FLASH_QT" not in os.environ:
        assert qt == want, f"T={T} heads={H}: the rule launched QT {qt}, expected {want}"
    ref, A = M.attn_ref(*M.split(qkv, H, 64), 0.125)
    W.add(f"rows QT{qt}", "sharp", M.check(out[0, :T], ref, M.flash_bar(ref, A, T), f"auto {shape}"), f"auto T={T} H={H}")
    qkv_d = qkv.to(G.DEV)
    vt = torch.full((H * 64 * ((T + 31) // 32 * 32),), G.NAN, dtype=F16, device=G.DEV)
    old = torch.full((T + G.GUARD, H * 64), G.NAN, dtype=F16, device=G.DEV)
    torch.cuda.synchronize()
    _lib.check(G.lib().gsv_op_flash_attn64(qkv_d.data_ptr(), T, H, 0.125, vt.data_ptr(), old.data_ptr(), None), "gsv_op_flash_attn64")
    torch.cuda.synchronize()
    assert G.last_route() == ("rows", qt)
    assert torch.equal(G.bits(old.cpu()[:T]), G.bits(out[0, :T])) and torch.isnan(old.cpu()[T:]).all()


@pytest.mark.parametrize("T", [33, 257])
def test_three_rows_hold_the_bits_of_each_row_alone(T):
    """rows = 3 with padded strides: QT is chosen from one row's size so that a row computes the same bits alone and in a batch"""
    for qt in (1, 2, 4):
        batch, _ = _rows(T, 2, "sharp", qt, seeds=(0, 1, 2))
        for r in range(3):
            alone, _ = _rows(T, 2, "sharp", qt, seeds=(r,))
            assert torch.equal(G.bits(batch[r]), G.bits(alone[0])), f"T={T} qt={qt}: row {r} differs from the row alone"


@pytest.mark.parametrize("T,H,half,rows", M.ROPE_CASES, ids=[f"T{t}_H{h}_half{p}_rows{r}" for t, h, p, r in M.ROPE_CASES])
def test_rotary_plane(T, H, half, rows):
    for qt in (1, 4):
        out, back = _rows(T, H, "sharp", qt, seeds=tuple(range(rows)), rope_half=half)
        if rows > 1:
            for r in range(rows):
                a_out, a_back = _rows(T, H, "sharp", qt, seeds=(r,), rope_half=half)
                assert torch.equal(G.bits(out[r]), G.bits(a_out[0])) and torch.equal(G.bits(back[r]), G.bits(a_back[0]))


# ---- segmented form --------------------------------------------------------------------------------------------------------

def _packed(lens):
    segs, o = [], 0
    for t in lens:
        segs.append((o, o + t))
        o += t
    return segs, o


@functools.lru_cache(maxsize=None)
def _seg_inputs(name, H, regime):
    lens = M.SEGS[name]
    segs, T = _packed(lens)
    qkv = M.make_qkv(T, H, 64, regime, F16, segs=segs)
    return qkv, segs, M.seg_attn_ref(qkv, lens, H, 64, 0.125)


def _alone_bits(x, H, qt):
    """the sequence alone through the rows hook at the same QT (bits only: the rows tests hold that path to the mirror)"""
    from gsv import _lib
    rc, out, _, _, _ = G.rows_call([x], H, qt)
    _lib.check(rc, "rows hook")
    return out[0, :x.shape[0]]


@pytest.mark.parametrize("name", list(M.SEGS))
def test_segments_every_qt(name):
    from gsv import _lib
    lens, H = M.SEGS[name], 2
    for regime in M.REGIMES:
        qkv, segs, (ref, A, n) = _seg_inputs(name, H, regime)
        if regime == "adversarial" and len(lens) > 1:   # a bad input, not a kernel failure: pick another seed
            q, k, _ = M.split(qkv, H, 64)
            assert M.hidden_mass_fraction(q, k, 0.125, M.self_ranges(segs, qkv.shape[0])) >= 0.9
        for qt in (1, 2, 4):
            what = f"seg {name} qt={qt} {regime}"
            rc, out, guard, vt = G.seg_call(qkv, lens, H, qt)
            _lib.check(rc, what)
            assert G.last_route() == ("seg", qt), what
            assert torch.isnan(guard).all() and torch.isfinite(vt).all(), what
            W.add(f"seg QT{qt}", regime, M.check(out, ref, M.flash_bar(ref, A, n), what), what)
            rc, out2, guard2, _ = G.seg_call(qkv, lens, H, qt)
            _lib.check(rc, what)
            assert torch.equal(G.bits(out2), G.bits(out)) and torch.isnan(guard2).all(), f"{what}: second launch differs"
            if regime != "flat" or name != "many":      # 40 equal lengths: one regime's worth of single launches is enough
                for lo, hi in segs:
                    assert torch.equal(G.bits(out[lo:hi]), G.bits(_alone_bits(qkv[lo:hi], H, qt))), \
                        f"{what}: segment [{lo}, {hi}) differs from the sequence alone"


def test_segment_hook_with_qt_0_is_the_existing_op_and_segments_are_isolated():
    from gsv import _lib
    lens, H = M.SEGS["second_trip"], 3
    qkv, segs, (ref, A, n) = _seg_inputs("second_trip", H, "sharp")
    rc, out, guard, _ = G.seg_call(qkv, lens, H, 0)
    _lib.check(rc, "seg qt 0")
    fam, qt = G.last_route()
    assert fam == "seg"
    W.add(f"seg QT{qt}", "sharp", M.check(out, ref, M.flash_bar(ref, A, n), "seg H=3"), "seg second_trip H=3 qt=0")
    rc, old, _, _ = G.seg_call(qkv, lens, H, None)
    _lib.check(rc, "gsv_op_flash_attn64_seg")
    assert G.last_route() == ("seg", qt) and torch.equal(G.bits(old), G.bits(out))
    # isolation: other values in ONE segment leave every other segment's output bit-identical
    lo, hi = segs[1]
    other = qkv.clone()
    other[lo:hi] = M.make_qkv(hi - lo, H, 64, "sharp", F16, seed=9)
    rc, out2, _, _ = G.seg_call(other, lens, H, 0)
    _lib.check(rc, "seg qt 0")
    keep = torch.ones(qkv.shape[0], dtype=torch.bool)
    keep[lo:hi] = False
    assert torch.equal(G.bits(out2[keep]), G.bits(out[keep])) and not torch.equal(G.bits(out2[~keep]), G.bits(out[~keep]))


# ---- refusals ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", M.ROWS_REFUSALS, ids=[c[0] for c in M.ROWS_REFUSALS])
def test_rows_refusals_leave_the_outputs_untouched(case):
    l = G.lib()
    _, present, T, heads, rows, rope, rope_half, qt, msg = case
    qkv = torch.zeros(64, 3 * 128, dtype=F16, device=G.DEV)
    vt = torch.full((1 << 16,), G.NAN, dtype=F16, device=G.DEV)
    out = torch.full((64 + G.GUARD, 128), G.NAN, dtype=F16, device=G.DEV)
    cs = torch.zeros(64, 64, 2, device=G.DEV)
    torch.cuda.synchronize()
    ptr = [t.data_ptr() if p else None for t, p in zip((qkv, vt, out), present)]
    l.gsv_debug_last_attn_route(1)
    rc = l.gsv_op_flash_attn64_rows(ptr[0], T, heads, rows, 0.125, cs.data_ptr() if rope else None, rope_half, qt, ptr[1], ptr[2], None)
    torch.cuda.synchronize()
    assert rc != 0 and msg in l.gsv_last_error().decode()
    assert l.gsv_debug_last_attn_route(1) == 0
    assert torch.isnan(vt).all() and torch.isnan(out).all() and not qkv.any()


def test_seg_refusal_of_an_unknown_qt_leaves_the_outputs_untouched():
    l = G.lib()
    qkv = torch.zeros(8, 3 * 128, dtype=F16, device=G.DEV)
    vt = torch.full((1 << 14,), G.NAN, dtype=F16, device=G.DEV)
    out = torch.full((8 + G.GUARD, 128), G.NAN, dtype=F16, device=G.DEV)
    torch.cuda.synchronize()
    l.gsv_debug_last_attn_route(1)
    rc = l.gsv_op_flash_attn64_seg_qt(qkv.data_ptr(), 2, G.ints([5, 3]), 2, 0.125, 3, vt.data_ptr(), out.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc != 0 and "qt 3" in l.gsv_last_error().decode() and l.gsv_debug_last_attn_route(1) == 0
    assert torch.isnan(vt).all() and torch.isnan(out).all()


def test_zz_worst_err_over_bar_table():
    """prints what the cases above measured (the figures DESIGN.md quotes); the bars themselves are asserted per case"""
    W.report()
