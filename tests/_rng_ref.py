"""Host mirror of the AR sampler's counter RNG (csrc/t2s_sample.h sample_core; DESIGN.md section 4d, "The counter RNG as a
contract") and the statistics the sampler tests share.  This file is the definition the tests pin; it is restated from the
kernel's code, not derived from its output:

    key  = (row << 40) ^ (step << 20) ^ v                       (64-bit; row < 2**24, step < 2**20, v < 2**20)
    hsh  = splitmix64(seed ^ splitmix64(key))
    u24  = hsh >> 40                                            (24 bits; u = u24 / 2**24 in [0, 1), exact in fp32)
    q    = max(-log1p(-u), 1e-20)                               (Exp(1); the clamp only bites at u24 == 0)

and token v of a row wins the race with score p[v] / q[v].  Everything is numpy uint64 (wrapping) and float64, broadcast
over seed / row / step and vectorised over v.

Bars.  chi2_bar(df) is the 1 - 1e-6 quantile of chi-square by Wilson-Hilferty; corr_bar(n) is 5 / sqrt(n), five standard
deviations of a sample correlation of independent streams.  The seeds of the tests are fixed, so a test either always passes or
always fails; the bars say how unlikely the pass would be for a broken generator, not how often a test flakes.
"""
import math

import numpy as np

M64 = (1 << 64) - 1
U24_MAX = (1 << 24) - 1
CLAMP = 1e-20


def _u64(x):
    """any integer (Python int of any sign or size, or integer array) as uint64 modulo 2**64"""
    if isinstance(x, (int, np.integer)):
        return np.uint64(int(x) & M64)
    a = np.asarray(x)
    if a.dtype == np.uint64:
        return a
    if a.dtype == object:
        return np.array([int(t) & M64 for t in a.reshape(-1)], dtype=np.uint64).reshape(a.shape)
    return a.astype(np.int64).astype(np.uint64)


def splitmix64(x):
    x = _u64(x)
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def splitmix64_int(x: int) -> int:
    """the same function on a plain Python int: the check of the uint64 arithmetic above"""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def uniform24_int(seed: int, row: int, step: int, v: int) -> int:
    key = ((row << 40) ^ (step << 20) ^ v) & M64
    return splitmix64_int((seed & M64) ^ splitmix64_int(key)) >> 40


def key(row, step, v):
    """the 64-bit counter of token v of (row, step); the three broadcast against each other"""
    with np.errstate(over="ignore"):
        return (_u64(row) << np.uint64(40)) ^ (_u64(step) << np.uint64(20)) ^ _u64(v)


def uniform24_of(seed, k):
    """hsh >> 40 for a seed and ready-made counters k (the negative controls build their own)"""
    return splitmix64(_u64(seed) ^ splitmix64(k)) >> np.uint64(40)


def uniform24(seed, row, step, V):
    """uint64 [..., V]: the 24-bit integers of tokens 0 .. V - 1; seed, row and step are scalars or arrays that broadcast"""
    seed, row, step = (np.asarray(_u64(t))[..., None] for t in (seed, row, step))
    return uniform24_of(seed, key(row, step, np.arange(V, dtype=np.uint64)))


def exp1(u24):
    """float64 q = max(-log1p(-u), 1e-20) of the 24-bit integers u24"""
    return np.maximum(-np.log1p(-(np.asarray(u24).astype(np.float64) / 16777216.0)), CLAMP)


def noise(seed, row, step, V):
    """float64 [..., V]: the Exp(1) draws of the race"""
    return exp1(uniform24(seed, row, step, V))


# ---- statistics ---------------------------------------------------------------------------------------------------------
def normal_quantile(p: float) -> float:
    """z with Phi(z) = p, by bisection on erfc (no dependency); |error| < 1e-12"""
    lo, hi = -40.0, 40.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if 0.5 * math.erfc(-mid / math.sqrt(2.0)) < p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def chi2_bar(df: int, tail: float = 1e-6) -> float:
    """the 1 - tail quantile of chi-square with df degrees of freedom (Wilson-Hilferty)"""
    z = normal_quantile(1.0 - tail)
    a = 2.0 / (9.0 * df)
    return df * (1.0 - a + z * math.sqrt(a)) ** 3


def corr_bar(n: int) -> float:
    return 5.0 / math.sqrt(n)


def corr(a, b) -> float:
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    a = a - a.mean()
    b = b - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


def chi2_uniform(u24, bins: int = 256):
    """(statistic, df) of the 24-bit integers over `bins` equal bins (bins a power of two)"""
    u = np.asarray(u24).reshape(-1)
    shift = 24 - int(math.log2(bins))
    cnt = np.bincount((u >> np.uint64(shift)).astype(np.int64), minlength=bins).astype(np.float64)
    e = u.size / bins
    return float(((cnt - e) ** 2 / e).sum()), bins - 1


def softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(x - x.max())
    return e / e.sum()


def chi2_counts(counts, p, min_expected: float = 5.0):
    """(statistic, df) of observed token counts against N p; tokens whose expected count is under min_expected share one bin"""
    counts = np.asarray(counts, dtype=np.float64)
    e = counts.sum() * np.asarray(p, dtype=np.float64)
    small = e < min_expected
    obs, exp = counts[~small], e[~small]
    if small.any():
        obs, exp = np.append(obs, counts[small].sum()), np.append(exp, e[small].sum())
    keep = exp > 0
    return float(((obs[keep] - exp[keep]) ** 2 / exp[keep]).sum()), int(keep.sum()) - 1


def race_logits(V: int = 64, scale: float = 1.5, seed: int = 5):
    """the fixed logits of the frequency tests, fp32 values"""
    return (np.random.default_rng(seed).standard_normal(V) * scale).astype(np.float32)


def race_winners(p, q):
    """argmax(p / q) along the last axis, first index on ties"""
    return np.argmax(np.asarray(p, dtype=np.float64) / q, axis=-1)
