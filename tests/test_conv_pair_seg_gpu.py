"""GPU: the masked fused ResBlock pair of a segmented decode (gsv_op_conv_pair_seg, conv_pair.hip SEG) against the path it
replaces: convs1 -> zero the gap rows -> convs2 -> zero the gap rows, as two gsv_op_conv1d launches with the row pass
restated in torch between and after them."""
import numpy as np
import pytest
import torch

from test_ops_gpu import DEV, _conv

pytestmark = pytest.mark.gpu

SEG_FLAG = 16


def _route():
    """(family, C, taps, flags) of the last launch; clears the record"""
    from gsv import _lib
    code = int(_lib.lib().gsv_debug_last_conv_route(1)) & 0xFFFFFFFFFFFFFFFF
    return code & 255, (code >> 16) & 255, (code >> 24) & 255, (code >> 56) & 255


def _row_seg(T, gaps):
    """segment ids 0, 1, 2, ... with -1 in the half-open row ranges `gaps`"""
    m = np.zeros(T, np.int32)
    sid, prev = 0, 0
    for a, b in sorted(gaps):
        m[prev:a] = sid
        m[a:b] = -1
        sid, prev = sid + 1, b
    m[prev:] = sid
    return m


def _gaps(T):
    """a segment of 3 rows at row 0, a gap across the first tile edge (row 256), a gap inside tile 1's intermediate halo (rows
    512 .. 512 + h2 belong to tile 1's 288-row image and to tile 2's body), a gap inside a tile, and a 3-row last segment"""
    want = [(3, 9), (250, 262), (513, 517), (700, 726), (T - 9, T - 3)]
    out = []
    for a, b in want:
        if 0 < a < b < T and (not out or a > out[-1][1]):
            out.append((a, b))
    return out


def _pack(w, C_, k):
    return w.permute(0, 2, 1).reshape(C_, k * C_).contiguous().to(DEV, torch.float16)


def _case(C_, k, dil, T, accum, seed_extra=0):
    torch.manual_seed(C_ * 100 + k * 10 + dil + seed_extra)
    x = torch.randn(C_, T)
    w1, w2 = torch.randn(C_, C_, k) / (C_ * k) ** 0.5, torch.randn(C_, C_, k) / (C_ * k) ** 0.5
    b1, b2 = torch.randn(C_) * 0.1, torch.randn(C_) * 0.1
    y0 = torch.randn(C_, T) if accum else None
    return x, w1, b1, w2, b2, y0


def _fused(fn_name, x, w1, b1, w2, b2, y0, T, C_, k, dil, scale, row_seg):
    """the op on a y buffer with 64 NaN sentinel rows after row T; returns (y [C, T] fp32 cpu, the sentinel rows)"""
    from gsv import _lib
    _lib.init(0)
    xd = x.t().contiguous().to(DEV, torch.float16)
    w1d, w2d, b1d, b2d = _pack(w1, C_, k), _pack(w2, C_, k), b1.to(DEV), b2.to(DEV)
    yd = torch.full((T + 64, C_), float("nan"), device=DEV, dtype=torch.float16)
    yd[:T] = y0.t().to(DEV, torch.float16) if y0 is not None else 0
    args = [xd.data_ptr(), w1d.data_ptr(), b1d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), yd.data_ptr(), T, C_, k, dil, scale,
            1 if y0 is not None else 0]
    if fn_name == "gsv_op_conv_pair_seg":
        rs = torch.from_numpy(row_seg).to(DEV) if row_seg is not None else None
        args.append(rs.data_ptr() if rs is not None else None)
    torch.cuda.synchronize()
    _lib.lib().gsv_debug_last_conv_route(1)
    _lib.check(getattr(_lib.lib(), fn_name)(*args, None), fn_name)
    torch.cuda.synchronize()
    return yd[:T].float().cpu().t(), yd[T:].cpu()


@pytest.mark.parametrize("C_,k,dil,T,accum", [(16, 3, 1, 256, True), (16, 7, 3, 1025, False), (16, 11, 5, 3000, False),
                                              (16, 11, 1, 200000, True), (16, 3, 5, 4500, False),
                                              (32, 11, 5, 2111, True), (32, 7, 1, 777, False), (32, 3, 5, 40000, False),
                                              (32, 11, 3, 5000, False), (32, 7, 3, 1300, True)])
def test_masked_pair_matches_two_launches_with_row_passes(C_, k, dil, T, accum):
    x, w1, b1, w2, b2, y0 = _case(C_, k, dil, T, accum)
    seg = _row_seg(T, _gaps(T))
    gap = torch.from_numpy(seg < 0)
    assert gap.any() and not gap[0] and not gap[-1]
    if not accum:
        x[:, gap] = 0                       # the mask contract: the input holds 0 in its gap rows
    # with accumulate the residual (x) and the accumulate operand stay NON-zero in the gap rows: they must still come out 0
    scale = 1.0 / 3.0 if accum else 1.0
    xh = x.half().float()
    t = _conv(xh, w1, b1, torch.float16, dil=dil, pre_lrelu=0.1)
    t[:, gap] = 0                                                                   # the row pass after convs1
    two = _conv(t, w2, b2, torch.float16, dil=1, pre_lrelu=0.1, res=xh, scale=scale,
                accumulate=y0.half().float() if accum else None)
    two[:, gap] = 0                                                                 # the row pass after convs2
    fused, tail = _fused("gsv_op_conv_pair_seg", x, w1, b1, w2, b2, y0, T, C_, k, dil, scale, seg)
    fam, c, taps, flags = _route()
    assert (fam, c, taps) == (8, C_, k) and flags & SEG_FLAG and bool(flags & 2) == accum, (fam, c, taps, flags)
    assert torch.isnan(tail).all(), "rows after T were written"
    assert not torch.isnan(fused).any()
    assert (fused[:, gap] == 0).all(), "a gap row of y is not 0"
    if accum:
        d = (fused - two).abs()
        share = (d > 0).float().mean().item()
        print(f"C={C_} k={k} dil={dil} T={T}: max diff {d.max().item():.3e}, differing share {share:.2e}")
        assert (d <= 1e-3 * (1 + two.abs())).all() and share < 1e-3
    else:
        assert torch.equal(fused, two), f"max diff {(fused - two).abs().max()}"
    # the mask matters: the unmasked pair on the same data differs next to a gap (its intermediate is not zeroed there)
    if not accum:
        plain, _ = _fused("gsv_op_conv_pair", x, w1, b1, w2, b2, y0, T, C_, k, dil, scale, None)
        assert not torch.equal(plain[:, ~gap], fused[:, ~gap])


@pytest.mark.parametrize("C_,k,dil,T,accum", [(16, 11, 5, 3000, False), (16, 7, 1, 1025, True), (32, 3, 3, 2111, False),
                                              (32, 11, 1, 40000, True)])
def test_map_without_gaps_equals_the_unmasked_pair(C_, k, dil, T, accum):
    x, w1, b1, w2, b2, y0 = _case(C_, k, dil, T, accum, seed_extra=5)
    scale = 1.0 / 3.0 if accum else 1.0
    plain, _ = _fused("gsv_op_conv_pair", x, w1, b1, w2, b2, y0, T, C_, k, dil, scale, None)
    fam, c, taps, flags = _route()
    assert (fam, c, taps) == (8, C_, k) and not flags & SEG_FLAG
    seg = np.zeros(T, np.int32)
    seg[T // 2:] = 1                                            # two segments, no gap row
    masked, tail = _fused("gsv_op_conv_pair_seg", x, w1, b1, w2, b2, y0, T, C_, k, dil, scale, seg)
    assert _route()[3] & SEG_FLAG
    assert torch.isnan(tail).all()
    assert torch.equal(masked, plain)


def test_bad_arguments_launch_nothing():
    from gsv import _lib
    C_, k, dil, T = 16, 7, 1, 1024
    x, w1, b1, w2, b2, _ = _case(C_, k, dil, T, False)
    seg = _row_seg(T, [(100, 130)])
    with pytest.raises(RuntimeError):
        _fused("gsv_op_conv_pair_seg", x, w1, b1, w2, b2, None, T, C_, k, dil, 1.0, None)       # row_seg = NULL: no fallback
    assert _route() == (0, 0, 0, 0)
    for bad_c, bad_k in [(48, k), (C_, 4)]:
        xd = torch.zeros(T, 64, device=DEV, dtype=torch.float16)
        wd = torch.zeros(64, 11 * 64, device=DEV, dtype=torch.float16)
        bd = torch.zeros(64, device=DEV)
        yd = torch.full((T, 64), 7.0, device=DEV, dtype=torch.float16)
        rs = torch.from_numpy(seg).to(DEV)
        _lib.lib().gsv_debug_last_conv_route(1)
        rc = _lib.lib().gsv_op_conv_pair_seg(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), wd.data_ptr(), bd.data_ptr(), yd.data_ptr(),
                                             T, bad_c, bad_k, dil, 1.0, 0, rs.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc != 0 and _route() == (0, 0, 0, 0)
        assert (yd == 7.0).all()
