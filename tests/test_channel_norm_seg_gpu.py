"""GPU: gsv_op_channel_norm_seg, the per-segment GroupNorm(C, C) of the packed HuBERT pass, against torch fp64 per segment.

Segments: conv 0's row ranges of the audios 400 / 719 / 8000 / 20800 laid out by HubertModel.pack_plan (79, 142, 1599 and 4159
rows at 64 k_s), and one segment of a single row.  C = 512.

Bars (output rounding plus fp32 partial sums; the statistics are finalised in double):
  fp16  |y - ref| <= 2^-10 |ref| + 1e-3      (half an ulp is 2^-11 |ref|; x itself arrives rounded to fp16, the reference reads the same x)
  fp32  |y - ref| <= 2e-5 (1 + |ref|)        (sums of up to 4159 fp32 terms, 64 per wave before the double-precision sum)
Inputs: per-channel means of up to 2.0 around deviations of 0.06 to 0.5 (mean / std up to 34), where E[x^2] - mean^2 from
unshifted fp32 sums cancels: the first version of the kernel missed the fp32 bar 5.3-fold there (max-abs 2.6e-4) and sums
x minus the segment's first row since.
Measured on an MI355X, largest |y - ref| / bar: fp16 0.33 (max-abs 9.8e-4, output rounding), fp32 0.051 (1.9e-6); one-row segment
0.014 / 0.000; the whole array against gsv_op_channel_norm 0.49 (fp16) / 0.015 (fp32)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACT_NONE, ACT_GELU = 0, 7
CH = 512
AUDIOS = (400, 719, 8000, 20800)


def _segments():
    from gsv.feature_extractor.cnhubert import HubertModel
    p = HubertModel.pack_plan(AUDIOS)
    return p["cn_start"], p["cn_len"], p["rows0"]


def _scratch(lens):
    return torch.full((2 * CH * (sum((t + 255) // 256 for t in lens) + len(lens)),), float("nan"), dtype=torch.float32, device=DEV)


def _call(x, starts, lens, gamma, beta, act, y, scratch=None, T=None, n_seg=None):
    from gsv import _lib
    _lib.init(0)
    n = len(starts) if n_seg is None else n_seg
    scratch = _scratch(lens) if scratch is None else scratch
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    a = (C.c_int32 * max(len(starts), 1))(*starts)
    b = (C.c_int32 * max(len(lens), 1))(*lens)
    return _lib.lib().gsv_op_channel_norm_seg(x.data_ptr(), x.shape[0] if T is None else T, x.shape[1], n, a, b, gamma.data_ptr(),
                                              beta.data_ptr(), 1e-5, act, scratch.data_ptr(), y.data_ptr(), _lib.dtype_code(x.dtype),
                                              st)


def _reference(x, starts, lens, gamma, beta, act):
    x, g, b = x.double().cpu(), gamma.double().cpu(), beta.double().cpu()
    ref = torch.zeros_like(x)
    for a, n in zip(starts, lens):
        seg = x[a:a + n]
        v = (seg - seg.mean(0)) / torch.sqrt(seg.var(0, unbiased=False) + 1e-5) * g + b
        ref[a:a + n] = torch.nn.functional.gelu(v) if act == ACT_GELU else v
    return ref


def _inputs(rows, dtype, tag="cn_seg", offset=2.0):
    from gsv import synthetic as S
    # a per-channel offset and scale, so that mean and variance differ from channel to channel: deviations of 0.06 to 0.5 around
    # means of up to `offset` (mean / std up to 34 at 2.0: E[x^2] - mean^2 would cancel in fp32)
    x = S.hash_symmetric(tag, (rows, CH), 1.0, 3) * (0.5 + S.hash_symmetric(tag + ".s", (CH,), 0.4, 3)) + S.hash_symmetric(tag + ".m", (CH,), offset, 3)
    gamma = (1.0 + S.hash_symmetric(tag + ".g", (CH,), 0.1, 3)).to(DEV, torch.float32)
    beta = S.hash_symmetric(tag + ".b", (CH,), 0.1, 3).to(DEV, torch.float32)
    return x.to(DEV, dtype).contiguous(), gamma, beta


def _within(y, ref, dtype):
    d = (y.double().cpu() - ref).abs()
    bar = 2.0 ** -10 * ref.abs() + 1e-3 if dtype == torch.float16 else 2e-5 * (1 + ref.abs())
    return d.max().item(), (d / bar).max().item()


@pytest.mark.parametrize("act", [ACT_GELU, ACT_NONE])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_segments_match_fp64_reference(dtype, act):
    starts, lens, rows = _segments()
    x, gamma, beta = _inputs(rows, dtype)
    y = torch.full_like(x, float("nan"))
    from gsv import _lib
    _lib.check(_call(x, starts, lens, gamma, beta, act, y), "gsv_op_channel_norm_seg")
    torch.cuda.synchronize()
    ref = _reference(x, starts, lens, gamma, beta, act)
    err, frac = _within(y, ref, dtype)
    print(f"[cnorm_seg] {dtype} act {act}: max-abs {err:.3e}, largest error / bar {frac:.3f}")
    assert frac <= 1.0
    # rows outside every segment are exactly 0 (y arrived as NaN)
    inside = torch.zeros(rows, dtype=torch.bool)
    for a, n in zip(starts, lens):
        inside[a:a + n] = True
    assert int(inside.sum()) < rows
    assert bool((y.cpu()[~inside] == 0).all()) and bool(torch.isfinite(y).all())


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_single_row_segment(dtype):
    """a segment of one row: variance 0, y = act(beta) there and 0 elsewhere"""
    x, gamma, beta = _inputs(40, dtype, "cn_one")
    y = torch.full_like(x, float("nan"))
    from gsv import _lib
    _lib.check(_call(x, [17], [1], gamma, beta, ACT_GELU, y), "gsv_op_channel_norm_seg")
    ref = _reference(x, [17], [1], gamma, beta, ACT_GELU)
    err, frac = _within(y, ref, dtype)
    print(f"[cnorm_seg] one row {dtype}: max-abs {err:.3e}, largest error / bar {frac:.3f}")
    assert frac <= 1.0
    assert bool((y[:17] == 0).all()) and bool((y[18:] == 0).all())


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_segment_bits_do_not_depend_on_neighbours_or_position(dtype):
    """segments A, B, C in one call, then C and A at other offsets in another: A's and C's rows are bit-equal"""
    from gsv import _lib
    la, lb, lc = 1599, 142, 4159
    xa, gamma, beta = _inputs(la, dtype, "cn_a")
    xb = _inputs(lb, dtype, "cn_b")[0]
    xc = _inputs(lc, dtype, "cn_c")[0]
    s1 = [0, 1664, 1920]
    x1 = torch.zeros(s1[2] + lc + 5, CH, dtype=dtype, device=DEV)
    for a, t in zip(s1, (xa, xb, xc)):
        x1[a:a + t.shape[0]] = t
    s2 = [3, 3 + lc + 70]                         # C first, A behind it, neither at a multiple of the chunk or of the row tile
    x2 = torch.zeros(s2[1] + la + 1, CH, dtype=dtype, device=DEV)
    x2[s2[0]:s2[0] + lc] = xc
    x2[s2[1]:s2[1] + la] = xa
    y1, y2 = torch.full_like(x1, float("nan")), torch.full_like(x2, float("nan"))
    _lib.check(_call(x1, s1, [la, lb, lc], gamma, beta, ACT_GELU, y1), "gsv_op_channel_norm_seg")
    _lib.check(_call(x2, s2, [lc, la], gamma, beta, ACT_GELU, y2), "gsv_op_channel_norm_seg")
    torch.cuda.synchronize()
    assert torch.equal(y1[s1[0]:s1[0] + la], y2[s2[1]:s2[1] + la])
    assert torch.equal(y1[s1[2]:s1[2] + lc], y2[s2[0]:s2[0] + lc])
    assert bool(torch.isfinite(y1).all()) and bool(torch.isfinite(y2).all())


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_whole_array_matches_channel_norm(dtype):
    """one segment over the whole array: within the same bar of gsv_op_channel_norm's result.  That op is no fp64 truth: it takes
    E[x^2] - mean^2 from unshifted fp32 partial sums, which costs y about (mean / std)^2 x 2e-7 x |y|, so it is itself within the
    fp32 bar only up to mean / std of about 10.  The comparison therefore runs at means of up to 0.2 (mean / std <= 3.5, like conv
    0's output, whose channels are close to zero-mean), not at the 34 of the fp64 comparisons above."""
    from gsv import _lib
    rows = 4159
    x, gamma, beta = _inputs(rows, dtype, "cn_whole", offset=0.2)
    y = torch.full_like(x, float("nan"))
    _lib.check(_call(x, [0], [rows], gamma, beta, ACT_GELU, y), "gsv_op_channel_norm_seg")
    y0 = torch.empty_like(x)
    scratch = torch.empty(128 * CH, dtype=torch.float32, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().gsv_op_channel_norm(x.data_ptr(), rows, CH, gamma.data_ptr(), beta.data_ptr(), 1e-5, ACT_GELU,
                                              scratch.data_ptr(), y0.data_ptr(), _lib.dtype_code(dtype), st), "gsv_op_channel_norm")
    torch.cuda.synchronize()
    err, frac = _within(y, y0.double().cpu(), dtype)
    print(f"[cnorm_seg] whole array vs gsv_op_channel_norm {dtype}: max-abs {err:.3e}, largest error / bar {frac:.3f}")
    assert frac <= 1.0


def test_bad_segment_tables_are_refused():
    from gsv import _lib
    x, gamma, beta = _inputs(64, torch.float16, "cn_err")
    y = torch.zeros_like(x)
    scratch = _scratch([64, 64, 64])
    GSV_ERR_ARG = -1
    err = _lib.lib().gsv_last_error
    assert _call(x, [0], [8], gamma, beta, ACT_NONE, y, scratch, n_seg=0) != 0                 # n_seg < 1
    assert _call(x, [0, 10], [8, 0], gamma, beta, ACT_NONE, y, scratch) != 0 and b"length" in err()
    assert _call(x, [0, 6], [8, 8], gamma, beta, ACT_NONE, y, scratch) != 0 and b"ascending" in err()     # overlapping
    assert _call(x, [20, 0], [8, 8], gamma, beta, ACT_NONE, y, scratch) != 0 and b"ascending" in err()    # descending
    assert _call(x, [0, 60], [8, 8], gamma, beta, ACT_NONE, y, scratch) != 0                   # ends past T
    assert _call(x, [0, 8], [8, 8], gamma, beta, ACT_NONE, y, scratch) == 0                    # touching segments are disjoint
    torch.cuda.synchronize()
    assert _call(x, [0], [8], gamma, beta, ACT_NONE, y, scratch, n_seg=0) == GSV_ERR_ARG
