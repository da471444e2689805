"""CPU: the host mirror of the sampler's counter RNG (tests/_rng_ref.py) has the properties production relies on.

* the uint64 arithmetic equals a plain Python-int implementation;
* noise() is Exp(1): mean, variance, and u uniform over 256 bins;
* argmax(p / q) samples the softmax;
* the streams of the best_of stride (row + 1024), of the next step, of the next seed and of one lane's neighbouring tokens
  (v and v + 64) are uncorrelated;
* negative controls on the mirror: q = u, a key without row and a key without step each exceed the bars, so the bars have teeth;
* the key space: rows alias modulo 2**24, and (row < 2**24, step < 2**20, v < 2**20) is injective.

Bars (see _rng_ref): chi-square at its 1 - 1e-6 quantile, correlations at 5 / sqrt(n), the mean of n Exp(1) draws at
5 / sqrt(n) and their variance at 5 sqrt(8 / n) (the variance of (q - 1)**2 is mu4 - 1 = 8).  All seeds are fixed.
tests/test_sampler_rng_gpu.py holds the kernel to this mirror.
"""
import math

import numpy as np

import _rng_ref as R

SEED = 0x8000000180000003          # bits 63, 32, 31 and the low bits set


def test_uint64_arithmetic_equals_python_ints():
    xs = [0, 1, 11, 1234, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0x100000000, 0x8000000000000000, R.M64, 0x9E3779B97F4A7C15]
    got = R.splitmix64(np.array(xs, dtype=np.uint64))
    assert [int(g) for g in got] == [R.splitmix64_int(x) for x in xs]
    assert int(R.splitmix64(R.M64)) == R.splitmix64_int(R.M64)
    for seed in (11, 0x80000000, SEED, R.M64):
        for row, step in ((0, 0), (63, 1), (2051, 1499), ((1 << 24) - 1, (1 << 20) - 1)):
            u = R.uniform24(seed, row, step, 2048)
            for v in (0, 1, 63, 64, 1023, 2047):
                assert int(u[v]) == R.uniform24_int(seed, row, step, v), (seed, row, step, v)
    # broadcasting: [rows][steps][V]
    u = R.uniform24(SEED, np.arange(3)[:, None], np.array([0, 7]), 5)
    assert u.shape == (3, 2, 5) and int(u[2, 1, 4]) == R.uniform24_int(SEED, 2, 7, 4)
    q = R.noise(SEED, 2, 7, 5)
    assert q.dtype == np.float64 and q[4] == max(-math.log1p(-R.uniform24_int(SEED, 2, 7, 4) / 2.0 ** 24), 1e-20)
    assert R.exp1(np.array([0], dtype=np.uint64))[0] == 1e-20
    assert abs(R.exp1(np.array([R.U24_MAX], dtype=np.uint64))[0] - 24 * math.log(2.0)) < 1e-12


def test_chi_square_bar_is_the_quantile():
    # Wilson-Hilferty against tabulated 0.999 quantiles (df 100: 149.449, df 250: 324.832) and the normal quantile itself
    assert abs(R.normal_quantile(0.975) - 1.959964) < 1e-6
    assert abs(R.chi2_bar(100, tail=1e-3) - 149.449) < 0.2
    assert abs(R.chi2_bar(250, tail=1e-3) - 324.832) < 0.3
    assert R.chi2_bar(255) > R.chi2_bar(255, tail=1e-3) > 255


def _shape_stats(q):
    n = q.size
    return abs(q.mean() - 1.0), 5.0 / math.sqrt(n), abs(q.var() - 1.0), 5.0 * math.sqrt(8.0 / n)


def test_noise_is_exponential():
    u = R.uniform24(SEED, np.arange(1024), 3, 2048)            # 2 097 152 values
    n = u.size
    assert n >= 2_000_000
    dm, bm, dv, bv = _shape_stats(R.exp1(u))
    x2, df = R.chi2_uniform(u, 256)
    print(f"[rng mirror] n = {n}: |mean - 1| = {dm:.2e} (bar {bm:.2e}), |var - 1| = {dv:.2e} (bar {bv:.2e}), "
          f"chi-square of u over 256 bins = {x2:.1f} (bar {R.chi2_bar(df):.1f}, df {df})")
    assert dm <= bm and dv <= bv
    assert x2 <= R.chi2_bar(df)
    # negative control: q = u instead of -log1p(-u)
    dm, bm, dv, bv = _shape_stats(u.astype(np.float64) / 2.0 ** 24)
    print(f"[rng mirror] control q = u: |mean - 1| = {dm:.3f}, |var - 1| = {dv:.3f}")
    assert dm > bm and dv > bv


def _race(q):
    """chi-square of the winners of len(q) races over the fixed logits against N * softmax"""
    p = R.softmax64(R.race_logits())
    counts = np.bincount(R.race_winners(p, q), minlength=p.size)
    return R.chi2_counts(counts, p)


def test_the_race_samples_the_softmax():
    rows, steps, V = np.arange(128)[:, None], np.arange(128), 64
    u = R.uniform24(SEED, rows, steps, V).reshape(-1, V)       # 16384 keys
    assert u.shape[0] >= 16384
    x2, df = _race(R.exp1(u))
    print(f"[rng mirror] race over {u.shape[0]} keys: chi-square = {x2:.1f} (bar {R.chi2_bar(df):.1f}, df {df})")
    assert x2 <= R.chi2_bar(df)
    # negative controls: q = u; a key without the row; a key without the step
    v = np.arange(V, dtype=np.uint64)
    controls = {
        "q = u": u.astype(np.float64) / 2.0 ** 24 + 2.0 ** -25,
        "key without row": R.exp1(R.uniform24_of(SEED, R.key(0 * rows[..., None], steps[..., None], v)).reshape(-1, V)),
        "key without step": R.exp1(R.uniform24_of(SEED, R.key(rows[..., None], 0 * steps[..., None], v)).reshape(-1, V)),
    }
    for name, q in controls.items():
        c2, cdf = _race(q)
        print(f"[rng mirror] control {name}: chi-square = {c2:.1f} (bar {R.chi2_bar(cdf):.1f})")
        assert c2 > R.chi2_bar(cdf), name


def test_streams_are_uncorrelated():
    rows, step, V = np.arange(1024), 17, 1024
    a = np.exp(-R.noise(SEED, rows, step, V))                  # exp(-q) = 1 - u: uniform
    n = a.size
    pairs = {
        "row + 1024 (best_of stride)": np.exp(-R.noise(SEED, rows + 1024, step, V)),
        "step + 1": np.exp(-R.noise(SEED, rows, step + 1, V)),
        "seed + 1": np.exp(-R.noise(SEED + 1, rows, step, V)),
    }
    for name, b in pairs.items():
        c = R.corr(a, b)
        print(f"[rng mirror] correlation with {name}: {c:+.2e} (bar {R.corr_bar(n):.2e}, n = {n})")
        assert abs(c) <= R.corr_bar(n), name
    lo, hi = a[:, :V - 64], a[:, 64:]
    c = R.corr(lo, hi)
    print(f"[rng mirror] correlation of tokens v and v + 64: {c:+.2e} (bar {R.corr_bar(lo.size):.2e}, n = {lo.size})")
    assert abs(c) <= R.corr_bar(lo.size)
    # negative controls: without the row in the key the best_of candidates share their noise, without the step every step does
    v = np.arange(V, dtype=np.uint64)
    no_row = lambda row, st: R.uniform24_of(SEED, R.key(0 * row[:, None], st, v))
    no_step = lambda row, st: R.uniform24_of(SEED, R.key(row[:, None], 0 * st, v))
    for name, ua, ub in (("key without row", no_row(rows, step), no_row(rows + 1024, step)),
                         ("key without step", no_step(rows, step), no_step(rows, step + 1))):
        c = R.corr(ua, ub)
        print(f"[rng mirror] control {name}: correlation {c:+.3f}")
        assert abs(c) > R.corr_bar(n), name


def test_key_space():
    # rows alias modulo 2**24 (row << 40 drops the upper bits): why gsv_t2s_set_row_rng refuses rows outside [0, 2**24)
    for r in (0, 5, 1027):
        assert np.array_equal(R.uniform24(SEED, r, 9, 256), R.uniform24(SEED, r + (1 << 24), 9, 256))
        assert not np.array_equal(R.uniform24(SEED, r, 9, 256), R.uniform24(SEED, r + (1 << 23), 9, 256))
    # the fields do not overlap inside their ranges ...
    edge = [(0, 0, 0), (0, 0, (1 << 20) - 1), (0, 1, 0), (0, (1 << 20) - 1, 0), (1, 0, 0), ((1 << 24) - 1, 0, 0),
            ((1 << 24) - 1, (1 << 20) - 1, (1 << 20) - 1), (0, (1 << 20) - 1, (1 << 20) - 1), (1, 0, (1 << 20) - 1)]
    keys = [int(R.key(*t)) for t in edge]
    assert len(set(keys)) == len(edge)
    assert int(R.key((1 << 24) - 1, (1 << 20) - 1, (1 << 20) - 1)) == R.M64
    # ... and do outside them
    assert int(R.key(0, 0, 1 << 20)) == int(R.key(0, 1, 0)) and int(R.key(0, 1 << 20, 0)) == int(R.key(1, 0, 0))
    # spot check: 10**6 random triples, as many distinct keys as distinct triples
    g = np.random.default_rng(3)
    row, step, v = g.integers(0, 1 << 24, 10 ** 6), g.integers(0, 1 << 20, 10 ** 6), g.integers(0, 1 << 20, 10 ** 6)
    k = R.key(row, step, v)
    triples = np.unique(np.stack([row, step, v], axis=1), axis=0).shape[0]
    assert np.unique(k).size == triples
    assert np.array_equal(k >> np.uint64(40), row.astype(np.uint64))
    assert np.array_equal((k >> np.uint64(20)) & np.uint64((1 << 20) - 1), step.astype(np.uint64))
    assert np.array_equal(k & np.uint64((1 << 20) - 1), v.astype(np.uint64))
    # splitmix64 is a bijection, so distinct keys give distinct inner hashes: spot check
    assert np.unique(R.splitmix64(k)).size == triples
