"""CPU: the fp64 mirror of the fused and materialised attention kernels and its bars (tests/_attnmirror.py) -- the mirror
against the independent restatements the repo already has (VitsOracle._rel_attention, the oracle's MRTE attention,
oracle/rope.py), each route's CPU emulation inside its bar over the GPU tests' shape tables, the mutants the bars must catch,
and the argument checks of the three hooks, which run before anything touches a device."""
import ctypes as C
import functools
import math

import pytest
import torch

import _attnmirror as M

F16 = torch.float16


# ---- the mirror is the oracle's attention --------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _oracle64():
    from oracle import cases
    from oracle.vits_oracle import VitsOracle
    vcfg, vsd, *_ = cases.vits_case_inputs(cases.VITS_CASES["vits_small"])
    orc = VitsOracle(vsd, vcfg)
    orc.sd = {k: v.double() for k, v in orc.sd.items()}
    return orc


@pytest.mark.parametrize("T", [1, 3, 9, 37])
def test_mirror_is_the_oracles_relative_attention(T):
    orc = _oracle64()
    prefix = "enc_p.encoder_ssl.attn_layers.0"
    C_ = orc.sd[prefix + ".conv_q.weight"].shape[1]
    nh, kc = orc.n_heads, C_ // orc.n_heads
    x = torch.randn(C_, T, generator=torch.Generator().manual_seed(T), dtype=torch.float64) * 4
    q, k, v = (orc.conv(x, f"{prefix}.conv_{n}").view(nh, kc, T).transpose(1, 2) for n in "qkv")
    rel_k, rel_v = orc.sd[prefix + ".emb_rel_k"][0], orc.sd[prefix + ".emb_rel_v"][0]
    ref, A = M.attn_ref(q, k, v, 1 / math.sqrt(kc), rel_k, rel_v)
    want = orc._rel_attention(x, prefix)
    assert torch.allclose(orc.conv(ref.t(), prefix + ".conv_o"), want, rtol=1e-10, atol=1e-10)
    assert (A >= ref.abs() - 1e-12).all()
    if T > 1:   # the band shifted by one offset must be visibly different: the pin is sensitive to the band's indexing
        bad, _ = M.attn_ref(q, k, v, 1 / math.sqrt(kc), rel_k.roll(1, 0), rel_v.roll(1, 0))
        assert (orc.conv(bad.t(), prefix + ".conv_o") - want).abs().max() > 1e-6


@pytest.mark.parametrize("Tq,Tk", [(1, 1), (5, 3), (9, 14)])
def test_mirror_is_the_oracles_mrte_attention(Tq, Tk):
    orc = _oracle64()
    p = "enc_p.mrte"
    g = torch.Generator().manual_seed(10 * Tq + Tk)
    ssl = torch.randn(orc.sd[p + ".c_pre.weight"].shape[1], Tq, generator=g, dtype=torch.float64) * 3
    text = torch.randn(orc.sd[p + ".text_pre.weight"].shape[1], Tk, generator=g, dtype=torch.float64) * 3
    ge = torch.randn(orc.sd[p + ".c_pre.weight"].shape[0], 1, generator=g, dtype=torch.float64)
    s, t = orc.conv(ssl, p + ".c_pre"), orc.conv(text, p + ".text_pre")
    Cc, nh = s.shape[0], 4
    kc = Cc // nh
    q = orc.conv(s, p + ".cross_attention.conv_q").view(nh, kc, Tq).transpose(1, 2)
    k = orc.conv(t, p + ".cross_attention.conv_k").view(nh, kc, Tk).transpose(1, 2)
    v = orc.conv(t, p + ".cross_attention.conv_v").view(nh, kc, Tk).transpose(1, 2)
    ref, _ = M.attn_ref(q, k, v, 1 / math.sqrt(kc))
    got = orc.conv(orc.conv(ref.t(), p + ".cross_attention.conv_o") + s + ge, p + ".c_post")
    assert torch.allclose(got, orc._mrte(ssl, text, ge), rtol=1e-10, atol=1e-10)


def test_mirror_ranges_are_block_attention_and_empty_rows_are_zero():
    """key ranges = the same attention run on each segment alone, with its own band; a gap row [t, t + 1) attends to itself
    (bias of offset 0, value v_t + rel_v[4]); an empty range gives 0 in ref and A"""
    segs, T = M.RANGE_LAYOUTS["short"]
    H, D = 2, 96
    qkv = M.make_qkv(T, H, D, "sharp", torch.float64, segs=segs)
    rel_k, rel_v = M.make_rel(D, "sharp")
    q, k, v = M.split(qkv, H, D)
    ref, A = M.attn_ref(q, k, v, 0.1, rel_k, rel_v, M.self_ranges(segs, T))
    for lo, hi in segs:
        alone, _ = M.attn_ref(q[:, lo:hi], k[:, lo:hi], v[:, lo:hi], 0.1, rel_k, rel_v)
        assert torch.allclose(ref[lo:hi], alone, rtol=1e-12, atol=1e-12)
    gap = 2
    assert torch.allclose(ref[gap], M.merge(v[:, gap:gap + 1] + rel_v[M.W].double())[0], rtol=1e-12, atol=1e-12)
    kr = M.cross_ranges([(0, 3)], [(2, 5)], 6)
    ref, A = M.attn_ref(q[:, :6], k[:, :9], v[:, :9], 0.1, kr=kr)
    assert not ref[3:].any() and not A[3:].any() and ref[:3].any()


@pytest.mark.parametrize("T,H,half", [(1, 2, 32), (33, 2, 32), (33, 16, 32), (40, 2, 12)])
def test_rotary_mirror_is_the_oracles(T, H, half):
    """interleaved pairs on the first 2 * half channels of the un-split projection (head 0 only at half = 32), the cos / sin
    table of RotaryEmbedding(64): against oracle/rope.py in float64, and the two mutants differ visibly"""
    from oracle.rope import RotaryEmbedding, apply_rotary_pos_emb
    freqs, _ = RotaryEmbedding(64).forward_from_seq_len(T)           # [1][T][64], interleaved duplicates
    cs32 = M.rope_table(T, half)
    want32 = torch.stack([freqs[0, :, 0:2 * half:2].cos(), freqs[0, :, 0:2 * half:2].sin()], dim=-1)
    assert torch.allclose(cs32, want32, rtol=0, atol=1e-6)
    f = freqs[..., :2 * half].double()
    cs = torch.stack([f[0, :, 0::2].cos(), f[0, :, 0::2].sin()], dim=-1)
    inner = H * 64
    qkv = torch.randn(T, 3 * inner, generator=torch.Generator().manual_seed(T + H), dtype=torch.float64)
    ref, bar = M.rope_ref(qkv, cs, half, H)
    for blk in (0, 1):
        want = apply_rotary_pos_emb(qkv[None, :, blk * inner:(blk + 1) * inner], f)[0]
        assert torch.allclose(ref[:, blk * inner:(blk + 1) * inner], want, rtol=1e-10, atol=1e-10)
    assert torch.equal(ref[:, 2 * inner:], qkv[:, 2 * inner:]) and not bar[:, 2 * inner:].any()
    assert not bar[:, 2 * half:inner].any() and (bar[:, :2 * half] > 0).all()
    if T > 1:
        for kw in (dict(pairing="half_split"), dict(every_head=True)):
            assert (M.rope_ref(qkv, cs, half, H, **kw)[0] - ref).abs().max() > 1e-2


# ---- inputs ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _self_case(T, H, D, regime, rel, layout=None, dtype=F16):
    segs = M.RANGE_LAYOUTS[layout][0] if layout else None
    qkv = M.make_qkv(T, H, D, regime, dtype, segs=segs)
    rel_k, rel_v = M.make_rel(D, regime, qkv=qkv, segs=segs, H=H) if rel else (None, None)
    kr = M.self_ranges(segs, T) if layout else None
    q, k, v = M.split(qkv, H, D)
    ref, A, pv = M.attn_ref(q, k, v, 1 / math.sqrt(D), rel_k, rel_v, kr, parts=True)
    return (q, k, v), (rel_k, rel_v), kr, (ref, A, pv)


def test_regimes_are_what_they_claim():
    pmax = {}
    for regime in ("flat", "sharp"):
        (q, k, v), _, _, _ = _self_case(300, 2, 64, regime, False)
        assert v.abs().max() <= 1.0
        pmax[regime] = torch.softmax(q.double() @ k.double().transpose(1, 2) / 8, -1).max(-1).values.median().item()
    assert pmax["flat"] < 0.05 and 0.3 < pmax["sharp"], pmax
    # the sharp band bias moves the argmax of one row in twenty or more
    (q, k, v), (rel_k, _), _, _ = _self_case(300, 2, 96, "sharp", True)
    s = q.double() @ k.double().transpose(1, 2) / math.sqrt(96)
    r, band = M._band_index(300, 300)
    b = (q.double() @ rel_k.double().t()) / math.sqrt(96)
    sb = s + torch.where(band, b.gather(2, r.clamp(0, 8).expand(2, 300, 300)), torch.zeros((), dtype=torch.float64))
    moved = (s.argmax(-1) != sb.argmax(-1)).float().mean().item()
    assert moved > 0.05, moved


@pytest.mark.parametrize("layout", list(M.RANGE_LAYOUTS))
def test_adversarial_ranges_put_the_mass_on_hidden_keys(layout):
    segs, T = M.RANGE_LAYOUTS[layout]
    (q, k, v), (rel_k, _), kr, _ = _self_case(T, 2, 96, "adversarial", True, layout)
    assert M.hidden_mass_fraction(q, k, 1 / math.sqrt(96), kr, rel_k) >= 0.9


@pytest.mark.parametrize("name", list(M.SEGS))
def test_adversarial_segments_put_the_mass_on_hidden_keys(name):
    lens = M.SEGS[name]
    if len(lens) < 2:
        return
    segs, T = _packed(lens)
    qkv = M.make_qkv(T, 2, 64, "adversarial", F16, segs=segs)
    q, k, _ = M.split(qkv, 2, 64)
    assert M.hidden_mass_fraction(q, k, 0.125, M.self_ranges(segs, T)) >= 0.9


def _packed(lens):
    segs, o = [], 0
    for t in lens:
        segs.append((o, o + t))
        o += t
    return tuple(segs), o


# ---- each emulation inside its bar over the whole shape table ----------------------------------------------------------------

def _report(name, worst):
    """Every bar here is a first-order worst-case bound of the route's rounding points, so an emulation of those points cannot
    leave it; how close it comes is printed (DESIGN.md quotes the figures).  The flash routes stay near 0.5-0.7; the
    materialised fp16 route reaches 0.94 on rows with two or three visible keys, where the fp16 rounding of P and of the
    output can both land near their worst case at once."""
    print(f"[attn_mirror] emulation, {name}: worst err/bar {worst:.3f}")
    assert worst <= 1.0, "the bar does not cover this route's own arithmetic"


@pytest.mark.parametrize("regime", ["flat", "sharp"])
def test_flash64_emulation_inside_the_flash_bar(regime):
    worst = 0.0
    cases = [(T, 2, 16) for T in M.ROWS_T] + [(T, h, 16) for T, h in M.ROWS_HEADS] + [(385, 2, 64), (129, 2, 32)]
    cases += [(t, 2, 16) for t in sorted({t for lens in M.SEGS.values() for t in lens})]
    for T, H, bq in sorted(set(cases)):
        (q, k, v), _, _, (ref, A, _) = _self_case(T, H, 64, regime, False)
        out = M.flash_emulate(q, k, v, 0.125, bq=bq)
        worst = max(worst, M.check(out, ref, M.flash_bar(ref, A, T), f"d64 {regime} T={T} H={H}"))
    _report(f"flash d=64 {regime}", worst)


@pytest.mark.parametrize("regime", ["flat", "sharp"])
def test_rel96_emulation_inside_the_flash_bar(regime):
    worst = 0.0
    for T, H in [(T, 2) for T in M.REL_T] + [(33, 3)]:
        (q, k, v), (rel_k, rel_v), _, (ref, A, _) = _self_case(T, H, 96, regime, True)
        out = M.flash_emulate(q, k, v, 1 / math.sqrt(96), rel_k, rel_v, bq=32)
        worst = max(worst, M.check(out, ref, M.flash_bar(ref, A, T), f"rel96 {regime} T={T} H={H}"))
    _report(f"flash d=96 with the band {regime}", worst)


@pytest.mark.parametrize("regime", M.REGIMES)
def test_rel96_range_emulation_inside_the_flash_bar(regime):
    worst = 0.0
    for layout, (segs, T) in M.RANGE_LAYOUTS.items():
        (q, k, v), (rel_k, rel_v), kr, (ref, A, _) = _self_case(T, 2, 96, regime, True, layout)
        out = M.flash_emulate(q, k, v, 1 / math.sqrt(96), rel_k, rel_v, kr, bq=32)
        worst = max(worst, M.check(out, ref, M.flash_bar(ref, A, T), f"rel96 ranges {regime} {layout}"))
    _report(f"flash d=96 with key ranges {regime}", worst)


def _mat_bar(dtype, ref, A, pv, Tk, rel):
    return M.mat_f16_bar(ref, A, pv, Tk, rel) if dtype == F16 else M.mat_f32_bar(ref)


@pytest.mark.parametrize("dtype", [F16, torch.float32], ids=["f16", "f32"])
@pytest.mark.parametrize("regime", M.REGIMES)
def test_materialised_emulation_inside_its_bar(regime, dtype):
    worst = 0.0
    sa = [(T, 96, True, None) for T in M.MAT_SELF_T] + [(T, 64, False, None) for T in M.MAT_SELF_T]
    sa += [(T, 96, True, layout) for layout, (_, T) in M.RANGE_LAYOUTS.items()]
    for T, D, rel, layout in sa:
        if regime == "adversarial" and not layout:
            continue
        (q, k, v), (rel_k, rel_v), kr, (ref, A, pv) = _self_case(T, 2, D, regime, rel, layout, dtype)
        out = M.mat_emulate(q, k, v, 1 / math.sqrt(D), rel_k, rel_v, kr)
        worst = max(worst, M.check(out, ref, _mat_bar(dtype, ref, A, pv, T, rel), f"mat self {regime} T={T} D={D} {layout}"))
    for Tq, Tk in M.CROSS:
        q, kv, kr, (ref, A, pv) = M.cross_case(Tq, Tk, regime, dtype)
        k, v = kv
        out = M.mat_emulate(q, k, v, 1 / math.sqrt(128), kr=kr)
        assert not out[kr[:, 1] == kr[:, 0]].any()
        worst = max(worst, M.check(out, ref, _mat_bar(dtype, ref, A, pv, Tk, False), f"mat cross {regime} {(Tq, Tk)}"))
    _report(f"materialised {dtype} {regime}", worst)


@pytest.mark.parametrize("dtype", [F16, torch.float32], ids=["f16", "f32"])
def test_materialised_emulation_long_row(dtype):
    """Tk = 12300: the row is not cached in LDS on the device; here the softmax and the sums over that many keys"""
    q, (k, v), (rel_k, rel_v), kr, (ref, A, pv) = M.long_case(dtype)
    out = M.mat_emulate(q, k, v, 1 / math.sqrt(96), rel_k, rel_v, kr)
    _report(f"materialised long row {dtype}", M.check(out, ref, _mat_bar(dtype, ref, A, pv, M.LONG[1], True), "long"))


def test_rope_emulation_inside_its_bar():
    worst = 0.0
    for T, H, half, _ in M.ROPE_CASES:
        qkv = M.make_qkv(T, H, 64, "sharp", F16)
        cs = M.rope_table(T, half)
        ref, bar = M.rope_ref(qkv, cs, half, H)
        worst = max(worst, M.check(M.rope_emulate(qkv, cs, half, H), ref, bar, f"rope T={T} H={H} half={half}"))
    _report("rotary", worst)


# ---- mutants the bars must catch -----------------------------------------------------------------------------------------------

def _caught(out, ref, bar):
    with pytest.raises(AssertionError, match="outside the bar"):
        M.check(out, ref, bar)


@pytest.mark.parametrize("regime", ["flat", "sharp"])
@pytest.mark.parametrize("D", [64, 96])
def test_bar_catches_chunk_stride_16(D, regime):
    """stride 16 in the chunk loop drops chunks 8-15 of every 16: invisible up to 256 keys, far outside the bar from 257 on"""
    rel = D == 96
    for T, caught in ((256, False), (257, True), (640, True)):
        (q, k, v), (rel_k, rel_v), _, (ref, A, _) = _self_case(T, 2, D, regime, rel)
        out = M.flash_emulate(q, k, v, 1 / math.sqrt(D), rel_k, rel_v, bq=32, stride=16)
        if caught:
            _caught(out, ref, M.flash_bar(ref, A, T))
        else:
            M.check(out, ref, M.flash_bar(ref, A, T))


@pytest.mark.parametrize("D", [64, 96])
def test_bar_catches_one_key_of_300_hidden_from_one_query(D):
    (q, k, v), (rel_k, rel_v), _, (ref, A, _) = _self_case(300, 2, D, "flat", D == 96)
    bar = M.flash_bar(ref, A, 300)
    M.check(M.flash_emulate(q, k, v, 1 / math.sqrt(D), rel_k, rel_v, bq=32), ref, bar)
    _caught(M.flash_emulate(q, k, v, 1 / math.sqrt(D), rel_k, rel_v, bq=32, hide=(211, 157)), ref, bar)


@pytest.mark.parametrize("mutant", ["hi_inclusive", "lo_early", "band_unmasked"])
@pytest.mark.parametrize("layout", list(M.RANGE_LAYOUTS))
def test_bar_catches_range_mutants(layout, mutant):
    """`j <= hi`, `j >= lo - 1`, and a band key outside the range keeping its biased score: in the adversarial regime the extra
    key carries most of the row's mass"""
    segs, T = M.RANGE_LAYOUTS[layout]
    (q, k, v), (rel_k, rel_v), kr, (ref, A, _) = _self_case(T, 2, 96, "adversarial", True, layout)
    _caught(M.flash_emulate(q, k, v, 1 / math.sqrt(96), rel_k, rel_v, kr, bq=32, **{mutant: True}), ref, M.flash_bar(ref, A, T))


@pytest.mark.parametrize("kw", [dict(pairing="half_split"), dict(every_head=True)], ids=["half_split", "every_head"])
def test_bar_catches_rotary_mutants(kw):
    for T, H, half, _ in M.ROPE_CASES:
        if T == 1:
            continue      # position 0 turns by nothing: every pairing is the identity there
        qkv = M.make_qkv(T, H, 64, "sharp", F16)
        cs = M.rope_table(T, half)
        ref, bar = M.rope_ref(qkv, cs, half, H)
        _caught(M.rope_emulate(qkv, cs, half, H, **kw), ref, bar)


@pytest.mark.parametrize("D", [64, 96])
def test_bar_catches_two_fp16_ulps_in_one_element(D):
    """sharp only: where one key leads, |ref| and A are both close to |v| and the bar is just under two ulps of the output
    (DESIGN.md "Mirror and bars" gives the reason no such claim is made in the flat regime)"""
    T = 257
    (q, k, v), (rel_k, rel_v), _, (ref, A, _) = _self_case(T, 2, D, "sharp", D == 96)
    bar = M.flash_bar(ref, A, T)
    out = M.flash_emulate(q, k, v, 1 / math.sqrt(D), rel_k, rel_v, bq=32)
    M.check(out, ref, bar)
    r0 = 256
    c = int(ref[r0].abs().argmax())
    bad = out.clone()
    up = (out[r0, c].double() >= ref[r0, c]) == bool(out[r0, c] > 0)
    bad.view(torch.int16)[r0, c] += 2 if up else -2
    assert abs(float(bad[r0, c]) - float(ref[r0, c])) > abs(float(out[r0, c]) - float(ref[r0, c]))
    _caught(bad, ref, bar)


# ---- the hooks' argument checks (no device needed: every refusal comes before the first HIP call) -----------------------------

def _ints(v):
    return (C.c_int32 * len(v))(*v)


def _lib():
    from gsv import build, _lib
    build.build(verbose=False)
    return _lib.lib()


@pytest.mark.parametrize("case", M.ROWS_REFUSALS, ids=[c[0] for c in M.ROWS_REFUSALS])
def test_rows_hook_refuses_before_any_launch(case):
    l = _lib()
    _, present, T, heads, rows, rope, rope_half, qt, msg = case
    buf = torch.zeros(64, 1024)        # host memory: a refusal must not touch it, and without a device nothing could
    ptr = [buf.data_ptr() if p else None for p in present]
    l.gsv_debug_last_attn_route(1)
    rc = l.gsv_op_flash_attn64_rows(ptr[0], T, heads, rows, 0.125, buf.data_ptr() if rope else None, rope_half, qt, ptr[1], ptr[2], None)
    assert rc == -1, "GSV_ERR_ARG expected"
    assert msg in l.gsv_last_error().decode(), l.gsv_last_error().decode()
    assert not buf.any() and l.gsv_debug_last_attn_route(1) == 0


def test_seg_hook_refuses_an_unknown_qt_before_any_launch():
    l = _lib()
    buf = torch.zeros(64, 1024)
    for qt in (3, -1, 8):
        rc = l.gsv_op_flash_attn64_seg_qt(buf.data_ptr(), 2, _ints([5, 3]), 2, 0.125, qt, buf.data_ptr(), buf.data_ptr(), None)
        assert rc == -1 and f"qt {qt}" in l.gsv_last_error().decode()
    assert not buf.any()


@pytest.mark.parametrize("case", M.ATTN_REFUSALS, ids=[c[0] for c in M.ATTN_REFUSALS])
def test_attention_hook_refuses_before_any_launch(case):
    l = _lib()
    _, present, Tq, Tk, heads, kc, rel, kr, code, route, msg = case
    buf = torch.zeros(64, 1024)
    ptr = [buf.data_ptr() if p else None for p in present]
    rp, rv = (buf.data_ptr() if rel else None), (buf.data_ptr() if rel == 1 else None)
    hk = max(heads, 1) * kc
    l.gsv_debug_last_attn_route(1)
    rc = l.gsv_op_attention(ptr[0], 3 * hk, 0, ptr[1], 3 * hk, hk, 2 * hk, Tq, Tk, heads, kc, 0.1, rp, rv, _ints(kr) if kr else None,
                            code, route, ptr[2], hk, None)
    assert rc == -1, "GSV_ERR_ARG expected"
    assert msg in l.gsv_last_error().decode(), l.gsv_last_error().decode()
    assert not buf.any() and l.gsv_debug_last_attn_route(1) == 0
