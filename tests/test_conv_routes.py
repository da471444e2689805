"""CPU: the conv route table, the fp64 mirror and its bar (tests/_conv_routes.py, tests/_convref.py), and the conv_pair tap
check -- everything about the conv / GEMM route tests that does not need a device."""
import math

import pytest
import torch
import torch.nn.functional as F

import _convref as R
from _conv_routes import CASES, PAIR_CASES, REACHABLE, decode_route, pair, strip_xcd


def test_route_table_names_every_reachable_instantiation():
    named = {strip_xcd(c.route) for c in CASES} | {pair(c, k, a) for c, k, a, _, _ in PAIR_CASES}
    assert sorted(set(REACHABLE) - named) == [], "instantiations without a case"
    assert sorted(named - set(REACHABLE)) == [], "cases expecting an instantiation the dispatcher cannot launch"
    assert len(REACHABLE) == len(set(REACHABLE)) == 128
    assert len({c.name for c in CASES}) == len(CASES)
    # both XCD orders of the LDS GEMM are pinned
    assert {c.route[-5:] for c in CASES if c.route.startswith("gemm_lds<")} == {"XCD1>", "XCD2>"}


def test_route_decoder():
    def code(*b):
        return sum(v << (8 * i) for i, v in enumerate(b))
    assert decode_route(0) == "none"
    assert decode_route(code(5, 1, 2, 2, 2, 4, 128, 1)) == "conv_lds<f16,TM2,TN2,WM2,WN4,CC128,ALLW0,RES1,ACC0>"
    assert decode_route(code(5, 0, 1, 2, 1, 4, 16, 4 | 2)) == "conv_lds<f32,TM1,TN2,WM1,WN4,CC16,ALLW1,RES0,ACC1>"
    assert decode_route(code(4, 1, 8, 2, 0, 0, 0, 8)) == "gemm_lds<f16,RES0,WNT1,W8,XCD2>"
    assert decode_route(code(2, 1, 8, 0, 0, 0, 0, 8)) == "gemm_t64_f16<WNT1,SLAB128>"
    assert decode_route(code(6, 1, 64, 2, 1, 8, 0, 3)) == "conv_narrow_f16<CC64,TM2,TN1,WN8,RES1,ACC1>"
    assert decode_route(code(8, 1, 32, 11, 0, 0, 0, 2)) == "conv_pair_f16<C32,TAPS11,ACC1>"
    assert decode_route(code(7, 0, 1, 4, 1, 4)) == "conv_gemm<f32,TM1,TN4,WM1,WN4>"


def _all_fp16():
    v = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(torch.float16)
    return v[torch.isfinite(v)]


def test_mirror_preact_matches_torch_where_the_slope_is_exact():
    """fp16 leaky-ReLU max(v, fp16(v * fp16(s))) is torch's half leaky_relu when s is an fp16 number (0.5, 0.25, 0.01 is not)"""
    v = _all_fp16()
    for s in (0.5, 0.25, 0.125):
        assert torch.equal(R.pre_act(v, R.ACT_LRELU, s), F.leaky_relu(v.float(), s).half())
    assert torch.equal(R.pre_act(v, R.ACT_RELU, 0.0), F.relu(v))
    vf = torch.randn(10000, dtype=torch.float32)
    assert torch.equal(R.pre_act(vf, R.ACT_LRELU, 0.1), F.leaky_relu(vf, 0.1))


def test_mirror_preact_fp16_slope_differs_from_torch():
    """The generator's slope 0.1 is not an fp16 number: the kernels multiply by fp16(0.1) = 0.0999755859375, torch's half
    leaky_relu by the fp32 0.1.  The two disagree on about a fifth of the negative fp16 values, by one ulp each -- the reason
    the mirror restates the kernels' rounding instead of calling torch."""
    v = _all_fp16()
    k = R.pre_act(v, R.ACT_LRELU, 0.1).float()
    t = F.leaky_relu(v.float(), 0.1).half().float()
    diff = k != t
    assert not diff[v > 0].any()
    frac = diff[v < 0].float().mean().item()
    assert 0.05 < frac < 0.5, frac
    assert torch.all((k - t).abs()[diff] <= R.ulp(t[diff], torch.float16))


@pytest.mark.parametrize("stride,dil,pad,taps", [(1, 1, 1, 3), (2, 1, 1, 4), (1, 5, 25, 11), (1, 3, 0, 2)])
def test_mirror_conv_matches_torch_conv1d(stride, dil, pad, taps):
    g = torch.Generator().manual_seed(taps)
    x = torch.randn(1, 97, 24, generator=g, dtype=torch.float64)
    w = torch.randn(1, 20, taps, 24, generator=g, dtype=torch.float64)
    T_out = (97 + 2 * pad - dil * (taps - 1) - 1) // stride + 1
    acc, mag = R.conv_cl(x[0], w[0], T_out, stride, dil, pad)
    ref = F.conv1d(x[0].t()[None], w[0].permute(0, 2, 1), stride=stride, dilation=dil, padding=pad)[0].t()
    assert torch.allclose(acc, ref, rtol=1e-12, atol=1e-12)
    assert torch.all(mag >= acc.abs() - 1e-12)


def test_mirror_transposed_scatter_matches_conv_transpose1d():
    """polyphase restatement (dil = -1, u * Cout virtual channels, scatter row t u + p - pad) = ConvTranspose1d"""
    g = torch.Generator().manual_seed(7)
    u, k, Cin, Co, T = 4, 8, 16, 6, 25
    xt = torch.randn(T, Cin, generator=g, dtype=torch.float64)
    wt = torch.randn(Cin, Co, k, generator=g, dtype=torch.float64)
    taps, pad = -(-k // u), (k - u) // 2
    wv = torch.zeros(u * Co, taps, Cin, dtype=torch.float64)
    for p in range(u):
        for q in range(taps):
            if q * u + p < k:
                wv[p * Co:(p + 1) * Co, q, :] = wt[:, :, q * u + p].t()
    ref, _ = R.conv_mirror(x=xt[None], w=wv[None], bias=None, gate=None, res=None, y_prev=None, dtype=torch.float64,
                           out_dtype=torch.float32, T_out=T * u, T_virt=T + taps - 1, stride=1, dil=-1, pad=0, pre=R.ACT_NONE,
                           slope=0.0, post=R.ACT_NONE, scale=1.0, ups_u=u, ups_pad=pad)
    want = F.conv_transpose1d(xt.t()[None], wt, stride=u, padding=pad)[0].t()
    assert torch.allclose(ref[0], want, rtol=1e-12, atol=1e-12)


def test_bar_catches_two_ulps_in_one_element():
    """A kernel output equal to the correctly rounded fp64 result passes; the same output with one element of the last
    256-row tile moved by 2 fp16 ulps fails (fp16 output, 3 taps x 128 channels: the fp32 part of the bar is ~0.3 ulp at
    the largest outputs).  fp32 outputs cannot be held to 2 ulps: there the accumulation term dominates by design."""
    g = torch.Generator().manual_seed(11)
    T, Cin, Cout, taps = 700, 128, 64, 3
    x = torch.randn(1, T, Cin, generator=g).half()
    w = (torch.randn(1, Cout, taps, Cin, generator=g) / math.sqrt(taps * Cin)).half()
    b = torch.randn(Cout, generator=g) * 0.5
    res = torch.randn(1, T, Cout, generator=g).half()
    ref, bar = R.conv_mirror(x=x, w=w, bias=b, gate=None, res=res, y_prev=None, dtype=torch.float16, out_dtype=torch.float16,
                             T_out=T, T_virt=T, stride=1, dil=1, pad=1, pre=R.ACT_LRELU, slope=0.1, post=R.ACT_NONE, scale=1.0)
    good = ref.half()
    assert R.check(good, ref, bar) <= 0.5 + 1e-9
    tile = ref[0, 512:]
    i = int(tile.abs().argmax())
    t, c = 512 + i // Cout, i % Cout
    bad = good.clone()
    bad[0, t, c] = (bad[0, t, c].double() + 2 * R.ulp(bad[0, t, c].double(), torch.float16)).half()
    assert bar[0, t, c] < 2 * R.ulp(ref[0, t, c], torch.float16)
    with pytest.raises(AssertionError, match="outside the bar"):
        R.check(bad, ref, bar)


def _built_lib():
    from gsv import build, _lib
    build.build(verbose=False)
    return _lib


@pytest.mark.parametrize("dil", [1, 6])
def test_conv_pair_accepts_exactly_the_instantiated_tap_counts(dil):
    """gsv_op_conv_pair's argument check runs before anything touches a device: with null operands an accepted shape stops
    at launch_conv_pair's operand check, a refused one at the op's shape check.  The accepted tap counts must be exactly
    the instantiated kernels (3, 5, 7, 9, 11): any other count would run the 11-tap kernel over smaller weights."""
    _lib = _built_lib()
    l = _lib.lib()
    accepted = []
    for taps in range(-13, 16):
        l.gsv_debug_last_conv_route(1)
        rc = l.gsv_op_conv_pair(None, None, None, None, None, None, 1024, 16, taps, dil, 1.0, 0, None)
        msg = l.gsv_last_error().decode()
        assert rc != 0 and l.gsv_debug_last_conv_route(1) == 0
        if "null operand" in msg:
            accepted.append(taps)
        else:
            assert "op_conv_pair: C must be" in msg, msg
    want = [k for k in (3, 5, 7, 9, 11) if (k - 1) // 2 * dil <= 25]
    assert accepted == want
