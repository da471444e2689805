"""GPU: the engines' attention() alone (gsv_op_attention over csrc/engine.hip's own routing) against the float64 mirror of
tests/_attnmirror.py, element by element: route 1 = flash_rel96_f16_kernel (with and without per-query key ranges), route 2 =
the materialised path attention_mat<T> in fp16 and fp32 (self-attention with and without the band, MRTE's cross form with empty
ranges, the row of 12300 keys that softmax_rows_kernel does not cache), route 0 = what the engine takes.

Every launch asserts: `out` arrives NaN-filled; every element finite and inside the route's bar (flash: 2^-11 |ref| + 2^-11 A +
T 2^-25; materialised fp16: the same + 2^-11 |P v| when relv_add_kernel rounds a second time; fp32: 2e-5); the 64 guard rows
behind `out` still NaN; the route record names the family; a second launch bit-identical.  The two routes round differently, so
they are compared within the sum of their bars only."""
import functools
import os

import pytest
import torch

import _attn_gpu as G
import _attnmirror as M

pytestmark = pytest.mark.gpu
F16, F32 = torch.float16, torch.float32
W = G.Worst("attn_routes")
ROUTE = {1: "rel96", 2: "materialised"}


@functools.lru_cache(maxsize=None)
def _self_case(T, H, D, regime, rel, layout, dtype, empty_gaps=False):
    segs = M.RANGE_LAYOUTS[layout][0] if layout else None
    qkv = M.make_qkv(T, H, D, regime, dtype, segs=segs)
    rel_kv = M.make_rel(D, regime, qkv=qkv, segs=segs, H=H) if rel else (None, None)
    kr = M.self_ranges(segs, T) if layout else None
    if empty_gaps:
        kr[kr[:, 1] - kr[:, 0] == 1] = 0                       # gap rows [0, 0) instead of [t, t + 1)
        for lo, hi in segs:
            kr[lo:hi, 0], kr[lo:hi, 1] = lo, hi                # (one-row segments keep their range)
    return qkv, rel_kv, kr, M.attn_ref(*M.split(qkv, H, D), D ** -0.5, rel_kv[0], rel_kv[1], kr, parts=True)


def _bar(route, dtype, ref, A, pv, Tk, rel):
    if route == 1:
        return M.flash_bar(ref, A, Tk)
    return M.mat_f16_bar(ref, A, pv, Tk, rel) if dtype == F16 else M.mat_f32_bar(ref)


def _checked(call, route, name, regime, ref, bar, what):
    """the per-launch assertions on call() -> rc, out, guard"""
    from gsv import _lib
    rc, out, guard = call()
    _lib.check(rc, what)
    fam, qt = G.last_route()
    assert fam == ROUTE[route] and (route != 1 or qt == 2), f"{what}: the launch recorded {fam} QT {qt}"
    assert torch.isnan(guard).all(), f"{what}: guard rows behind out were written"
    W.add(name, regime, M.check(out, ref, bar, what), what)
    rc, out2, guard2 = call()
    _lib.check(rc, what)
    assert torch.equal(G.bits(out2), G.bits(out)) and torch.isnan(guard2).all(), f"{what}: second launch differs"
    return out


def _self(T, H, D, regime, rel, layout, dtype, route, empty_gaps=False):
    qkv, rel_kv, kr, (ref, A, pv) = _self_case(T, H, D, regime, rel, layout, dtype, empty_gaps)
    name = f"{ROUTE[route]} {'f16' if dtype == F16 else 'f32'}" + (" ranges" if layout else "")
    what = f"{name} T={T} H={H} kc={D} band={rel} layout={layout} {regime}"
    out = _checked(lambda: G.attn_call(qkv, None, H, D, route, rel_kv, kr, packed=True), route, name, regime, ref,
                   _bar(route, dtype, ref, A, pv, T, rel), what)
    return out, _bar(route, dtype, ref, A, pv, T, rel)


def _route0_equals(T, H, D, regime, rel, layout, dtype, want_route, out):
    """route 0 = what the engine would take, bit for bit (unless the A/B switch is set)"""
    from gsv import _lib
    qkv, rel_kv, kr, _ = _self_case(T, H, D, regime, rel, layout, dtype)
    rc, out0, guard = G.attn_call(qkv, None, H, D, 0, rel_kv, kr, packed=True)
    _lib.check(rc, "route 0")
    fam, _ = G.last_route()
    assert torch.isnan(guard).all()
    if "GSV_MATERIALIZED_ENC_ATTN" not in os.environ:
        assert fam == ROUTE[want_route] and torch.equal(G.bits(out0), G.bits(out)), f"route 0 is not route {want_route}"


# ---- route 1: the fused kernel -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", M.REL_T)
def test_rel96_without_ranges(T):
    for regime in ("flat", "sharp"):
        out, _ = _self(T, 2, 96, regime, True, None, F16, 1)
    _route0_equals(T, 2, 96, "sharp", True, None, F16, 1, out)


def test_rel96_three_heads_and_the_existing_op():
    from gsv import _lib
    T, H = 33, 3
    out, _ = _self(T, H, 96, "sharp", True, None, F16, 1)
    qkv, (rel_k, rel_v), _, _ = _self_case(T, H, 96, "sharp", True, None, F16)
    qkv_d, rk, rv = qkv.to(G.DEV), rel_k.to(G.DEV), rel_v.to(G.DEV)
    vt = torch.full((H * 96 * 64,), G.NAN, dtype=F16, device=G.DEV)
    old = torch.full((T + G.GUARD, H * 96), G.NAN, dtype=F16, device=G.DEV)
    torch.cuda.synchronize()
    _lib.check(G.lib().gsv_op_flash_rel96(qkv_d.data_ptr(), T, H, 96 ** -0.5, rk.data_ptr(), rv.data_ptr(), vt.data_ptr(), old.data_ptr(),
                                          None), "gsv_op_flash_rel96")
    torch.cuda.synchronize()
    assert torch.equal(G.bits(old.cpu()[:T]), G.bits(out)) and torch.isnan(old.cpu()[T:]).all()


@pytest.mark.parametrize("layout", list(M.RANGE_LAYOUTS))
def test_rel96_with_key_ranges_and_the_materialised_route_beside_it(layout):
    segs, T = M.RANGE_LAYOUTS[layout]
    for regime in M.REGIMES:
        qkv, (rel_k, _), kr, _ = _self_case(T, 2, 96, regime, True, layout, F16)
        if regime == "adversarial":      # a bad input, not a kernel failure: pick another seed
            q, k, _ = M.split(qkv, 2, 96)
            assert M.hidden_mass_fraction(q, k, 96 ** -0.5, kr, rel_k) >= 0.9
        o1, b1 = _self(T, 2, 96, regime, True, layout, F16, 1)
        o2, b2 = _self(T, 2, 96, regime, True, layout, F16, 2)
        assert ((o1.double() - o2.double()).abs() <= b1 + b2).all(), f"{layout} {regime}: the routes differ by more than both bars"
        _self(T, 2, 96, regime, True, layout, F32, 2)
    _route0_equals(T, 2, 96, "adversarial", True, layout, F16, 1, o1)


# ---- route 2: the materialised path ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
@pytest.mark.parametrize("T", M.MAT_SELF_T)
def test_materialised_self_attention(T, dtype):
    for regime in ("flat", "sharp"):
        _self(T, 2, 96, regime, True, None, dtype, 2)
        out, _ = _self(T, 2, 64, regime, False, None, dtype, 2)
    _route0_equals(T, 2, 64, "sharp", False, None, dtype, 2, out)
    if dtype == F32:
        out, _ = _self(T, 2, 96, "sharp", True, None, dtype, 2)
        _route0_equals(T, 2, 96, "sharp", True, None, dtype, 2, out)


@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
@pytest.mark.parametrize("Tq,Tk", M.CROSS)
def test_materialised_cross_attention_with_empty_ranges(Tq, Tk, dtype):
    for regime in M.REGIMES:
        q2, kv2 = M.cross_case_packed(Tq, Tk, regime, dtype)
        q, (k, v), kr, (ref, A, pv) = M.cross_case(Tq, Tk, regime, dtype)
        if regime == "adversarial":
            assert M.hidden_mass_fraction(q, k, 128 ** -0.5, kr) >= 0.9
        name = f"materialised {'f16' if dtype == F16 else 'f32'} cross"
        out = _checked(lambda: G.attn_call(q2, kv2, 4, 128, 2, kr=kr), 2, name, regime, ref, _bar(2, dtype, ref, A, pv, Tk, False),
                       f"{name} {(Tq, Tk)} {regime}")
        empty = kr[:, 1] == kr[:, 0]
        assert empty.any() and not G.bits(out[empty]).any(), "an empty range must give an exactly zero row"


@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_materialised_band_with_empty_ranges_gives_zero_rows(dtype):
    """gap rows [0, 0) under the band: P and the band probabilities are both zeroed, so relv_add_kernel adds nothing"""
    segs, T = M.RANGE_LAYOUTS["three"]
    out, _ = _self(T, 2, 96, "sharp", True, "three", dtype, 2, empty_gaps=True)
    _, _, kr, _ = _self_case(T, 2, 96, "sharp", True, "three", dtype, True)
    empty = kr[:, 1] == kr[:, 0]
    assert int(empty.sum()) == 10 and not G.bits(out[empty]).any()


@pytest.mark.parametrize("dtype", [F16, F32], ids=["f16", "f32"])
def test_materialised_row_of_12300_keys(dtype):
    """Tk > 12288: softmax_rows_kernel recomputes the biased, masked row instead of caching it in LDS"""
    q2, kv2 = M.long_case(dtype, packed=True)
    q, (k, v), rel, kr, (ref, A, pv) = M.long_case(dtype)
    name = f"materialised {'f16' if dtype == F16 else 'f32'} long"
    _checked(lambda: G.attn_call(q2, kv2, 1, 96, 2, rel, kr), 2, name, "sharp", ref, _bar(2, dtype, ref, A, pv, M.LONG[1], True), name)


# ---- refusals ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", M.ATTN_REFUSALS, ids=[c[0] for c in M.ATTN_REFUSALS])
def test_refusals_leave_the_outputs_untouched(case):
    l = G.lib()
    _, present, Tq, Tk, heads, kc, rel, kr, code, route, msg = case
    dtype = F16 if code == 1 else F32
    hk = max(heads, 1) * kc
    qkv = torch.zeros(16, 3 * hk, dtype=dtype, device=G.DEV)
    out = torch.full((16 + G.GUARD, hk), G.NAN, dtype=dtype, device=G.DEV)
    tab = torch.zeros(9, kc, device=G.DEV)
    torch.cuda.synchronize()
    ptr = [t.data_ptr() if p else None for t, p in zip((qkv, qkv, out), present)]
    rp, rv = (tab.data_ptr() if rel else None), (tab.data_ptr() if rel == 1 else None)
    l.gsv_debug_last_attn_route(1)
    rc = l.gsv_op_attention(ptr[0], 3 * hk, 0, ptr[1], 3 * hk, hk, 2 * hk, Tq, Tk, heads, kc, 0.1, rp, rv, G.ints(kr) if kr else None,
                            code, route, ptr[2], hk, None)
    torch.cuda.synchronize()
    assert rc != 0 and msg in l.gsv_last_error().decode()
    assert l.gsv_debug_last_attn_route(1) == 0 and torch.isnan(out).all()


def test_zz_worst_err_over_bar_table():
    """prints what the cases above measured (the figures DESIGN.md quotes); the bars themselves are asserted per case"""
    W.report()
