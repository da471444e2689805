"""fp64 mirror of the conv / GEMM launches (gsv_op_conv1d, gsv_op_conv_pair) with a per-element error bar derived from
the arithmetic, not tuned to any kernel.

What the kernels do, and what the mirror therefore does:
  * operands are stored in the engine dtype: x, w and the residual are rounded to it (fp32 residuals where requested);
  * the pre-activation runs in the operand dtype at load: fp16 leaky-ReLU is max(v, fp16(v * fp16(slope))) -- the slope
    is rounded to fp16 first, unlike torch's half leaky_relu, which multiplies by the fp32 slope (tests/test_conv_routes.py
    shows the difference); fp32 leaky-ReLU is max(v, v * slope) in fp32;
  * the contraction accumulates in fp32 (MFMA); the mirror sums in float64;
  * epilogue, in this order: (((acc + bias) * gate + res) * scale) -> post_act -> (+ y_prev), one rounding to the output
    dtype at the end.

Bar per output element:  |got - ref| <= ulp_out(|ref|) + 16 sqrt(K) 2^-24 S  (+ an absolute term for tanh / GELU / SiLU)
  K = taps * Cin (the contraction length); S = |scale| L (|gate| (sum_i |x_i w_i| + |b|) + |res|) + |y_prev|, the fp64 sum of
  the magnitudes that enter the element, L the activation's Lipschitz bound.  fp32 accumulation of K terms is good to
  about sqrt(K) 2^-24 S (16 = headroom for the few fp32 epilogue roundings and the MFMA's summation order); the rounding to
  the output dtype adds at most one ulp of the result once the fp32 value sits within an ulp of the exact one.
"""
from __future__ import annotations

import math

import torch

ACT_NONE, ACT_RELU, ACT_TANH, ACT_LRELU, ACT_SILU, ACT_GELU, ACT_GELU_TANH = 0, 1, 2, 3, 6, 7, 8
U32 = 2.0 ** -24
# Lipschitz bounds of the post activations: max |d/du| of SiLU = 1.0998, of GELU (erf or tanh form) = 1.1289
_LIP = {ACT_NONE: 1.0, ACT_RELU: 1.0, ACT_TANH: 1.0, ACT_SILU: 1.13, ACT_GELU: 1.13, ACT_GELU_TANH: 1.13}
# absolute error of the fp32 evaluation of the activation itself: the fast tanh (__expf, __fdividef) and expf / erff / tanhf
# are good to a few fp32 ulps of 1; 16 ulps of 1
_ACT_ABS = {ACT_TANH: 2.0 ** -20, ACT_SILU: 2.0 ** -20, ACT_GELU: 2.0 ** -20, ACT_GELU_TANH: 2.0 ** -20}


def ulp(v: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """unit in the last place of |v| in `dtype` (fp16 / fp32), subnormal range included"""
    a = v.abs().to(torch.float64)
    if dtype == torch.float16:
        mant, emin = 10, -14
    elif dtype == torch.float32:
        mant, emin = 23, -126
    else:
        raise ValueError(dtype)
    e = torch.floor(torch.log2(a.clamp_min(2.0 ** emin)))
    return torch.exp2(e - mant)


def pre_act(x: torch.Tensor, act: int, slope: float) -> torch.Tensor:
    """the load-time activation of the kernels on operands already stored in their dtype (fp16 / fp32), same dtype out"""
    if act == ACT_LRELU:
        if x.dtype == torch.float16:
            s = torch.tensor(slope, dtype=torch.float16)
            # fp16 x fp16 is exact in fp32 (22 significant bits), so one rounding to fp16 = the hardware fp16 multiply
            return torch.maximum(x, (x.float() * s.float()).half())
        return torch.maximum(x, x * torch.tensor(slope, dtype=torch.float32))
    if act == ACT_RELU:
        return x.clamp_min(0)
    if act == ACT_NONE:
        return x
    raise ValueError(act)


def post_act(u: torch.Tensor, act: int) -> torch.Tensor:
    if act == ACT_NONE:
        return u
    if act == ACT_RELU:
        return u.clamp_min(0)
    if act == ACT_TANH:
        return torch.tanh(u)
    if act == ACT_SILU:
        return u * torch.sigmoid(u)
    if act == ACT_GELU:
        return 0.5 * u * (1 + torch.erf(u / math.sqrt(2.0)))
    if act == ACT_GELU_TANH:
        return 0.5 * u * (1 + torch.tanh(math.sqrt(2.0 / math.pi) * (u + 0.044715 * u ** 3)))
    raise ValueError(act)


def conv_cl(x: torch.Tensor, w: torch.Tensor, T_virt: int, stride: int, dil: int, pad: int):
    """channels-last implicit GEMM in float64: x [T_in][Cin], w [Cout][taps][Cin] (fp64) ->
    acc[t][co] = sum_{tap,ci} x[t*stride + tap*dil - pad][ci] w[co][tap][ci] (rows outside [0, T_in) are zero), and the same
    sum over magnitudes.  Any dil (negative: the polyphase restatement of a transposed conv)."""
    T_in = x.shape[0]
    t = torch.arange(T_virt)
    acc = torch.zeros(T_virt, w.shape[0], dtype=torch.float64)
    mag = torch.zeros_like(acc)
    xa, wa = x.abs(), w.abs()
    for tap in range(w.shape[1]):
        rows = t * stride + tap * dil - pad
        ok = ((rows >= 0) & (rows < T_in)).to(torch.float64)[:, None]
        idx = rows.clamp(0, T_in - 1)
        acc += (x[idx] * ok) @ w[:, tap, :].t()
        mag += (xa[idx] * ok) @ wa[:, tap, :].t()
    return acc, mag


def conv_mirror(*, x, w, bias, gate, res, y_prev, dtype, out_dtype, T_out, T_virt, stride, dil, pad, pre, slope, post, scale,
                ups_u=0, ups_pad=0, bz=0):
    """Reference of one gsv_op_conv1d launch over Z slices.

    x [Z][T_in][Cin] and w [Z][Cout][taps][Cin] in the engine dtype; bias / gate fp32 [Z*bz or Cout_real] or None; res
    [Z][T_out][Cout_real] in its stored dtype or None; y_prev [Z][T_out][Cout_real] in out_dtype or None (accumulate).
    Returns (ref, bar) float64 [Z][T_out][Cout_real]."""
    Z, Cout = x.shape[0], w.shape[1]
    cr = Cout // ups_u if ups_u else Cout
    K = w.shape[2] * w.shape[3]
    ref = torch.zeros(Z, T_out, cr, dtype=torch.float64)
    bar = torch.zeros_like(ref)
    written = torch.zeros(Z, T_out, cr, dtype=torch.bool)
    for z in range(Z):
        xin = pre_act(x[z], pre, slope).to(torch.float64)
        acc, mag = conv_cl(xin, w[z].to(torch.float64), T_virt, stride, dil, pad)
        if ups_u:
            t = torch.arange(T_virt)[:, None]
            c = torch.arange(Cout)[None, :]
            p, oc = c // cr, c % cr
            orow = (t * ups_u + p - ups_pad).expand(T_virt, Cout)
            oc = oc.expand(T_virt, Cout)
            keep = (orow >= 0) & (orow < T_out)
            a_s = torch.zeros(T_out, cr, dtype=torch.float64)
            m_s = torch.zeros_like(a_s)
            a_s[orow[keep], oc[keep]] = acc[keep]
            m_s[orow[keep], oc[keep]] = mag[keep]
            written[z][orow[keep], oc[keep]] = True
            acc, mag = a_s, m_s
        else:
            acc, mag = acc[:T_out], mag[:T_out]
            written[z] = True
        b = torch.zeros(cr, dtype=torch.float64) if bias is None else bias[z * bz:z * bz + cr].to(torch.float64)
        g = torch.ones(cr, dtype=torch.float64) if gate is None else gate[z * bz:z * bz + cr].to(torch.float64)
        u = (acc + b) * g
        s = g.abs() * (mag + b.abs())
        if res is not None:
            r = res[z].to(torch.float64)
            u = u + r
            s = s + r.abs()
        u = post_act(u * scale, post)
        s = s * abs(scale) * _LIP[post]
        if y_prev is not None:
            yp = y_prev[z].to(torch.float64)
            u = u + yp
            s = s + yp.abs()
        ref[z] = u
        bar[z] = ulp(u, out_dtype) + 16 * math.sqrt(K) * U32 * s + _ACT_ABS.get(post, 0.0) * (1 + u.abs())
    assert written.all(), "the scatter leaves output elements unwritten: the case is malformed"
    return ref, bar


def lrelu16(v: torch.Tensor, slope: float = 0.1) -> torch.Tensor:
    return pre_act(v, ACT_LRELU, slope)


def pair_mirror(*, x, w1, b1, w2, b2, dil, scale, y_prev):
    """Reference of one fused ResBlock pair (gsv_op_conv_pair): y = (convs2(lrelu(convs1(lrelu(x)))) + x) * scale [+ y_prev].
    x [T][C] fp16, w1 / w2 [C][taps][C] fp16, b1 / b2 fp32 [C], y_prev [T][C] fp16 or None.

    The kernel rounds the intermediate convs1(...) + b1 to fp16 before its leaky-ReLU (the two-launch path stores it), so the
    mirror does too.  Its fp32 value may sit on the other side of an fp16 rounding boundary: the intermediate can differ by
    eps1 + one ulp (eps1 = the fp32 bound of convs1), and that difference reaches the output through sum |w2|."""
    T, Cc = x.shape
    taps = w1.shape[1]
    h2 = (taps - 1) // 2
    W1, W2 = w1.to(torch.float64), w2.to(torch.float64)
    acc1, mag1 = conv_cl(lrelu16(x).to(torch.float64), W1, T, 1, dil, h2 * dil)
    hp = acc1 + b1.to(torch.float64)
    eps1 = 16 * math.sqrt(taps * Cc) * U32 * (mag1 + b1.to(torch.float64).abs())
    h = lrelu16(hp.to(torch.float32).half()).to(torch.float64)
    acc2, mag2 = conv_cl(h, W2, T, 1, 1, h2)
    delta = eps1 + ulp(hp.abs() + eps1, torch.float16)
    prop, _ = conv_cl(delta, W2.abs(), T, 1, 1, h2)
    xf = x.to(torch.float64)
    u = (acc2 + b2.to(torch.float64) + xf) * scale
    s = (mag2 + b2.to(torch.float64).abs() + xf.abs()) * abs(scale)
    if y_prev is not None:
        u = u + y_prev.to(torch.float64)
        s = s + y_prev.to(torch.float64).abs()
    bar = ulp(u, torch.float16) + 16 * math.sqrt(taps * Cc) * U32 * s + abs(scale) * prop
    return u, bar


def check(got: torch.Tensor, ref: torch.Tensor, bar: torch.Tensor, what: str = "") -> float:
    """every element within its bar; returns the worst err / bar ratio"""
    err = (got.to(torch.float64) - ref).abs()
    ratio = err / bar
    worst = ratio.max().item()
    if not worst <= 1.0:      # NaN fails too
        i = int(torch.nan_to_num(ratio, nan=float("inf")).argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
        bad = int((~(ratio <= 1.0)).sum())
        raise AssertionError(f"{what}: {bad} element(s) outside the bar; worst at {idx}: got {got[idx].item()!r} ref "
                             f"{ref[idx].item()!r} err {err[idx].item():.3e} bar {bar[idx].item():.3e}")
    return worst
