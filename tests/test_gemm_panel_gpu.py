"""GPU: the prefill's panel GEMM (csrc/gemm_panel.hip) through gsv_op_gemm_panel.

For every tile of the family and each of the three epilogue forms, over M in {one tile, one tile + 1, two tiles - 1, 33, 1},
N in {one column tile, one column tile + 32, 512, 1536} and K in {64, 128, 512, 2048}:
  * byte-identical to gemm_lds.  At these small M the dispatcher would pick gemm_sk / gemm_t64, whose split-K sums differ, so the
    reference is always the same descriptor through gsv_op_conv1d with 2049 rows (the first M of them are the test's rows): its
    route is asserted to decode to gemm_lds before anything is compared.  A GEMM row does not depend on the other rows.
  * within the bar of the fp64 mirror (tests/_convref.py), the check test_conv_routes_gpu.py applies to gemm_lds;
  * rows >= M and 64 guard rows behind y keep their NaN sentinel, a second launch is bit-identical;
  * the route record reads family 9 with the tile's rows / 32 and columns / 32.
References are computed once per (N, K, form) and shared by the tiles.

Tile 4 is the 96 x 128 tile with gemm_t64's two-accumulator summation, the form the prefill takes where the dispatcher launches
gemm_t64 (up to 2048 rows): the same checks against the SAME descriptor through gsv_op_conv1d, whose route must decode to gemm_t64.
"""
import ctypes as C
import math
import zlib

import pytest
import torch

import _convref as R
from _conv_routes import decode_route
from _gemm_panel_cases import FORMS, GSV_ERR_ARG, GSV_F16, REFUSALS, ROUTE_GEMM_PANEL, T64_TILE, TILES, desc_fields, refusal_desc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
M_REF = 2049                                       # gemm_sk serves up to 2048 rows; from here on the dispatcher takes gemm_lds
M_MAX = 2 * 192 - 1                                # the most rows any case uses: the mirror covers these
KS = (64, 128, 512, 2048)
SENT = {torch.float16: (torch.int16, 0x7E5A), torch.float32: (torch.int32, 0x7FC0DEAD)}   # quiet NaNs no kernel writes


def _bits(t):
    return t.view(SENT[t.dtype][0])


def _sentinel(shape, dtype):
    it, v = SENT[dtype]
    return torch.full(shape, v, dtype=it, device=DEV).view(dtype)


_REFS = {}


def _reference(N, K, form):
    """operands of M_REF rows, gemm_lds' output for them, and the fp64 mirror + bar of the first M_MAX rows"""
    key = (N, K, form)
    if key in _REFS:
        return _REFS[key]
    from gsv import _lib
    _lib.init(0)
    out_f32, has_res, post = FORMS[form]
    g = torch.Generator()
    g.manual_seed(zlib.crc32(f"panel_{N}_{K}_{form}".encode()))
    x = torch.randn(M_REF, K, generator=g).half()
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half()
    bias = torch.randn(N, generator=g) * 0.5
    res = torch.randn(M_REF, N, generator=g).half() if has_res else None
    ydt = torch.float32 if out_f32 else torch.float16
    dev = dict(x=x.to(DEV), w=w.to(DEV), bias=bias.to(DEV), res=res.to(DEV) if has_res else None)
    y = _sentinel((M_REF, N), ydt)
    d = _lib.ConvDesc(x=dev["x"].data_ptr(), w=dev["w"].data_ptr(), bias=dev["bias"].data_ptr(), y=y.data_ptr(),
                      res=dev["res"].data_ptr() if has_res else None, **desc_fields(form, M_REF, K, N))
    _lib.lib().gsv_debug_last_conv_route(1)
    _lib.check(_lib.lib().gsv_op_conv1d(C.byref(d), GSV_F16, None), "reference launch")
    route = decode_route(_lib.lib().gsv_debug_last_conv_route(1))
    torch.cuda.synchronize()
    assert route.startswith("gemm_lds"), f"the reference of N={N} K={K} {form} ran on {route}, not on gemm_lds"
    ref, bar = R.conv_mirror(x=x[None, :M_MAX], w=w[None, :, None, :], bias=bias, gate=None, res=res[None, :M_MAX] if has_res else None,
                             y_prev=None, dtype=torch.float16, out_dtype=ydt, T_out=M_MAX, T_virt=M_MAX, stride=1, dil=1, pad=0,
                             pre=R.ACT_NONE, slope=0.1, post=post, scale=1.0)
    _REFS[key] = dict(dev=dev, y=y.cpu(), ref=ref[0], bar=bar[0], ydt=ydt, has_res=has_res)
    return _REFS[key]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("tile", list(TILES))
def test_gemm_panel_matches_gemm_lds_bit_for_bit(tile, form):
    from gsv import _lib
    _lib.init(0)
    l = _lib.lib()
    tr, tc = TILES[tile]
    compared = 0
    for N in (tc, tc + 32, 512, 1536):
        for K in KS:
            r = _reference(N, K, form)
            dev, ydt = r["dev"], r["ydt"]
            for M in (tr, tr + 1, 2 * tr - 1, 33, 1):
                what = f"tile {tile} {form} M={M} N={N} K={K}"
                outs = []
                for _ in range(2):
                    y = _sentinel((M + GUARD, N), ydt)
                    d = _lib.ConvDesc(x=dev["x"].data_ptr(), w=dev["w"].data_ptr(), bias=dev["bias"].data_ptr(), y=y.data_ptr(),
                                      res=dev["res"].data_ptr() if r["has_res"] else None, **desc_fields(form, M, K, N))
                    l.gsv_debug_last_conv_route(1)
                    _lib.check(l.gsv_op_gemm_panel(C.byref(d), GSV_F16, tile, None), what)
                    code = int(l.gsv_debug_last_conv_route(1))
                    torch.cuda.synchronize()
                    assert (code & 255, code >> 8 & 255, code >> 16 & 255, code >> 24 & 255) == (ROUTE_GEMM_PANEL, GSV_F16, tr // 32, tc // 32), \
                        f"{what}: route record {code:#x}"
                    assert (code >> 56 & 1) == int(r["has_res"]), f"{what}: RES flag of {code:#x}"
                    outs.append(y.cpu())
                assert torch.equal(_bits(outs[0]), _bits(outs[1])), f"{what}: second launch differs"
                assert torch.all(_bits(outs[0][M:]) == SENT[ydt][1]), f"{what}: rows >= M or guard rows written"
                got = outs[0][:M]
                assert torch.equal(_bits(got), _bits(r["y"][:M])), \
                    f"{what}: {int((_bits(got) != _bits(r['y'][:M])).sum())} element(s) differ from gemm_lds"
                R.check(got, r["ref"][:M], r["bar"][:M], what)
                compared += 1
    assert compared == 4 * len(KS) * 5


@pytest.mark.parametrize("form", list(FORMS))
def test_gemm_panel_t64_sum_matches_gemm_t64_bit_for_bit(form):
    from gsv import _lib
    _lib.init(0)
    l = _lib.lib()
    out_f32, has_res, post = FORMS[form]
    ydt = torch.float32 if out_f32 else torch.float16
    compared = 0
    for N, K in ((128, 512), (160, 512), (512, 512), (1536, 512), (2048, 512), (512, 2048)):
        g = torch.Generator()
        g.manual_seed(zlib.crc32(f"panel_t64_{N}_{K}_{form}".encode()))
        Mx = 278
        x = torch.randn(Mx, K, generator=g).half()
        w = (torch.randn(N, K, generator=g) / math.sqrt(K)).half()
        bias = torch.randn(N, generator=g) * 0.5
        res = torch.randn(Mx, N, generator=g).half() if has_res else None
        xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
        rd = res.to(DEV) if has_res else None
        ref, bar = R.conv_mirror(x=x[None], w=w[None, :, None, :], bias=bias, gate=None, res=res[None] if has_res else None, y_prev=None,
                                 dtype=torch.float16, out_dtype=ydt, T_out=Mx, T_virt=Mx, stride=1, dil=1, pad=0, pre=R.ACT_NONE,
                                 slope=0.1, post=post, scale=1.0)
        for M in (96, 97, 191, 33, 1, Mx):
            what = f"t64 sum {form} M={M} N={N} K={K}"
            outs = []
            for which in ("dispatcher", "panel", "panel"):
                y = _sentinel((M + GUARD, N), ydt)
                d = _lib.ConvDesc(x=xd.data_ptr(), w=wd.data_ptr(), bias=bd.data_ptr(), y=y.data_ptr(),
                                  res=rd.data_ptr() if has_res else None, **desc_fields(form, M, K, N))
                l.gsv_debug_last_conv_route(1)
                if which == "dispatcher":
                    _lib.check(l.gsv_op_conv1d(C.byref(d), GSV_F16, None), what)
                    route = decode_route(l.gsv_debug_last_conv_route(1))
                    assert route.startswith("gemm_t64"), f"{what}: the dispatcher ran {route}, not gemm_t64"
                else:
                    _lib.check(l.gsv_op_gemm_panel(C.byref(d), GSV_F16, T64_TILE, None), what)
                    code = int(l.gsv_debug_last_conv_route(1))
                    assert (code & 255, code >> 16 & 255, code >> 24 & 255, code >> 32 & 255) == (ROUTE_GEMM_PANEL, 3, 4, 1), f"{what}: {code:#x}"
                torch.cuda.synchronize()
                outs.append(y.cpu())
            assert torch.equal(_bits(outs[1]), _bits(outs[2])), f"{what}: second launch differs"
            assert torch.all(_bits(outs[1][M:]) == SENT[ydt][1]), f"{what}: rows >= M or guard rows written"
            assert torch.equal(_bits(outs[1][:M]), _bits(outs[0][:M])), \
                f"{what}: {int((_bits(outs[1][:M]) != _bits(outs[0][:M])).sum())} element(s) differ from gemm_t64"
            R.check(outs[1][:M], ref[0][:M], bar[0][:M], what)
            compared += 1
    assert compared == 36


def test_gemm_panel_launcher_choice_fills_one_round_at_the_prefill_shapes():
    """tile 0 = the launcher's choice: at M = 5760 each of the four prefill shapes runs as 240 workgroups on 256 CUs (>= 85 %)"""
    from gsv import _lib
    _lib.init(0)
    l = _lib.lib()
    M = 5760
    for K, N, form in ((512, 1536, "bias"), (512, 512, "bias_res_f32"), (512, 2048, "bias_relu"), (2048, 512, "bias_res_f32")):
        out_f32, has_res, _ = FORMS[form]
        x = torch.zeros(M, K, dtype=torch.float16, device=DEV)
        w = torch.zeros(N, K, dtype=torch.float16, device=DEV)
        b = torch.zeros(N, device=DEV)
        res = torch.zeros(M, N, dtype=torch.float16, device=DEV) if has_res else None
        y = torch.empty(M, N, dtype=torch.float32 if out_f32 else torch.float16, device=DEV)
        d = _lib.ConvDesc(x=x.data_ptr(), w=w.data_ptr(), bias=b.data_ptr(), y=y.data_ptr(), res=res.data_ptr() if has_res else None,
                          **desc_fields(form, M, K, N))
        l.gsv_debug_last_conv_route(1)
        _lib.check(l.gsv_op_gemm_panel(C.byref(d), GSV_F16, 0, None), f"{N}x{K}")
        code = int(l.gsv_debug_last_conv_route(1))
        torch.cuda.synchronize()
        assert code & 255 == ROUTE_GEMM_PANEL
        tr, tc = 32 * (code >> 16 & 255), 32 * (code >> 24 & 255)
        wgs = -(-M // tr) * -(-N // tc)
        assert 0.85 * 256 <= wgs <= 256, (N, K, tr, tc, wgs)


@pytest.mark.parametrize("name", list(REFUSALS))
def test_gemm_panel_refusals_leave_the_output_untouched(name):
    from gsv import _lib
    _lib.init(0)
    l = _lib.lib()
    M, K, N = 2304, 512, 512
    x = torch.zeros(M + 8, 3 * K, dtype=torch.float16, device=DEV)      # room for the taps-3 / offset-pointer forms
    w = torch.zeros(N + 8, 3 * K, dtype=torch.float16, device=DEV)
    b = torch.zeros(N, device=DEV)
    gate = torch.ones(N, device=DEV)
    res = torch.zeros(M, 1024, dtype=torch.float32, device=DEV)
    y = _sentinel((2 * M, 1024), torch.float32)                          # covers every output form of the table
    d, dtype, tile = refusal_desc(_lib, name, M, K, N, x=x.data_ptr(), w=w.data_ptr(), bias=b.data_ptr(), y=y.data_ptr(),
                                  res=res.data_ptr(), gate=gate.data_ptr())
    l.gsv_debug_last_conv_route(1)
    rc = l.gsv_op_gemm_panel(C.byref(d), dtype, tile, None)
    torch.cuda.synchronize()
    assert rc == GSV_ERR_ARG, (name, rc)
    assert l.gsv_debug_last_conv_route(1) == 0
    assert torch.all(_bits(y) == SENT[torch.float32][1]), f"{name}: a refused launch wrote to y"
