"""The fp64 mirror of gsv_op_resample_poly_seg (include/gsv.h): a direct loop over
    y[i] = sum_j h[i * down + half - j * up] * x[j],  j in [0, n) with the filter index in [0, L),  L = 2 * half + 1,
which is scipy.signal.resample_poly(x, up, down, window=h / up, padtype="constant") (tests/test_resample_plan.py).  Besides y it
returns, per output, S_i = sum |h x| and the tap count t_i: the terms of the fp32 error bar of tests/test_resample_op_gpu.py."""
from math import gcd

import numpy as np

RATE_PAIRS = [(32000, 16000), (48000, 16000), (44100, 16000), (44100, 32000), (16000, 32000), (22050, 16000), (24000, 32000)]


def up_down(sr_in, sr_out):
    g = gcd(sr_in, sr_out)
    return sr_out // g, sr_in // g


def out_len(n, up, down):
    return (n * up + down - 1) // down


def resample_mirror(x, h, up, down):
    """x [n], h [L] (any float dtype, used as fp64) -> (y [m], S [m], taps [m]) in fp64 / int"""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    n, L = x.shape[0], h.shape[0]
    assert L % 2 == 1
    half = L // 2
    m = out_len(n, up, down)
    y, S, taps = np.zeros(m), np.zeros(m), np.zeros(m, dtype=np.int64)
    for i in range(m):
        c = i * down + half
        ja = max(0, -((L - 1 - c) // up))            # ceil((c - (L - 1)) / up)
        jb = min(n - 1, c // up)
        if jb < ja:
            continue
        j = np.arange(ja, jb + 1)
        p = h[c - j * up] * x[j]
        y[i], S[i], taps[i] = p.sum(), np.abs(p).sum(), j.shape[0]
    return y, S, taps


def error_bar(ref, S, taps):
    """|y - ref| <= (t_i + 2) 2^-24 S_i + 2^-24 |ref|: fp32 accumulation of t_i products in any order (t_i - 1 additions, each
    within 2^-24 relative, plus the product's rounding) with a filter rounded to fp32 (one more 2^-24 on every term), and the
    rounding of the reference itself to the output format"""
    u = 2.0 ** -24
    return (taps + 2) * u * S + u * np.abs(ref)
