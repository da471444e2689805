"""Host mirrors of csrc/align.hip: the fp64 log-probabilities, the float64 monotonic alignment search with VITS' tie rule, a brute
force over every monotonic path, the proportional fallback, planted alignments, and the error bar of the fp32 log-probabilities.

The bar (absolute, per element of lp), derived for the kernel's arithmetic with u = 2**-24 and gamma_n = n u / (1 - n u):

  s = scale * <q_h[t], k_h[j]>.  The dot product is one fp32 accumulation chain over the d = head_dim products in k order (fp32
  operands: the fp32 MFMA is a chain of fmaf; fp16 operands: the 22-bit products are exact and the MFMA adds them into the fp32
  accumulator), then one multiplication by scale: |s^ - s| <= gamma_{d+2} scale A, A = sum_i |q_i k_i|.  Any order of the d
  additions obeys the same bound.
  softmax: with m^ = max_j s^ (exact), e_j = expf(s^_j - m^): the subtraction rounds once (<= u |s^_j - m^| <= 2 u max|s|), expf
  is within 1 ulp (2 u).  The shift cancels in the quotient, so numerator and denominator each carry a relative error of at most
  gamma_{d+2} scale A + 2 u max|s| + 2 u, the denominator also the (nl - 1) u of its additions in any order, the division 1 ulp.
  The mean over H heads adds H + 1 roundings, all terms positive.  Up to here a relative error of p, that is an absolute one of lp:
      2 gamma_{d+2} scale A + (nl + 4 max|s| + H + 8) u.
  logf is within 1 ulp of its result, which is stored in fp32: + ulp32(|lp|).  Terms of a head below 1e-37 (expf underflow) lose
  their relative accuracy; they matter only where every head is that small, and there max(1e-30, .) clamps both sides.
bar = 2 gamma_{d+2} scale max A + (nl + 4 max|s| + H + 16) u + ulp32(|lp|), the 16 in place of 8 for slack in the rounding count."""
import itertools

import numpy as np

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def logp_mirror(q, k, heads, scale):
    """q [nf][heads * d], k [nl][heads * d] (any float dtype, taken at their stored values) -> lp float64 [nf][nl], and the two
    operand statistics of the bar: max_htj sum_i |q_i k_i| and max |s|"""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    nf, nl = q.shape[0], k.shape[0]
    d = q.shape[1] // heads
    p = np.zeros((nf, nl))
    a_max = s_max = 0.0
    for h in range(heads):
        qh, kh = q[:, h * d:(h + 1) * d], k[:, h * d:(h + 1) * d]
        s = float(np.float32(scale)) * (qh @ kh.T)
        a_max = max(a_max, float((np.abs(qh) @ np.abs(kh).T).max()))
        s_max = max(s_max, float(np.abs(s).max()))
        e = np.exp(s - s.max(axis=1, keepdims=True))
        p += e / e.sum(axis=1, keepdims=True)
    return np.log(np.maximum(1e-30, p / heads)), a_max, s_max


def logp_bar(lp64, a_max, s_max, heads, d, scale):
    nl = lp64.shape[1]
    flat = 2.0 * gamma(d + 2) * float(scale) * a_max + (nl + 4.0 * s_max + heads + 16) * U
    return flat + np.spacing(np.abs(lp64).astype(np.float32)).astype(np.float64)


def searched(nf, nl):
    return nf >= 1 and nl >= 1 and nf >= nl and nl <= 1024


def fallback_ends(nf, nl):
    return np.array([((j + 1) * nf) // nl for j in range(nl)], np.int32)


def dp_mirror(lp, keep64=False):
    """lp fp32 [nf][nl] -> (ends int32 [nl], score float32, V float64 of the last row): the kernel's recurrence in float64, one
    add and one compare per cell, and its backtrack.  keep64: lp is float64 and stays so (the optimum under the fp64 mirror)"""
    lp = np.asarray(lp, np.float64 if keep64 else np.float32)
    nf, nl = lp.shape
    if not searched(nf, nl):
        return fallback_ends(nf, nl), np.float32(-np.inf), None
    V = np.full(nl, -np.inf)
    V[0] = np.float64(lp[0, 0])
    dec = np.zeros((nf, nl), bool)
    for t in range(1, nf):
        left = np.concatenate(([-np.inf], V[:-1]))
        take = V < left                      # a tie stays
        V = lp[t].astype(np.float64) + np.where(take, left, V)
        dec[t] = take
    ends = np.zeros(nl, np.int32)
    j = nl - 1
    ends[j] = nf
    for t in range(nf - 1, 0, -1):
        if j > 0 and (j == t or dec[t, j]):
            ends[j - 1] = t
            j -= 1
    return ends, np.float32(V[nl - 1] / np.float64(nf)), V


def path_of(ends, nf):
    """phoneme index of every frame"""
    ends = np.asarray(ends)
    return np.searchsorted(ends, np.arange(nf), side="right")


def path_sum(lp, ends):
    """sum of lp (any dtype, summed in float64) along the path `ends` describes; ends must be a monotonic path with >= 1 frame each"""
    lp = np.asarray(lp, np.float64)
    nf, nl = lp.shape
    e = np.asarray(ends, np.int64)
    assert e.shape == (nl,) and e[-1] == nf and e[0] >= 1 and np.all(np.diff(e) >= 1), "not a monotonic path over every phoneme"
    return float(lp[np.arange(nf), path_of(e, nf)].sum())


def all_paths(nf, nl):
    """every monotonic path as its ends vector: the compositions of nf into nl positive parts"""
    for cuts in itertools.combinations(range(1, nf), nl - 1):
        yield np.array(list(cuts) + [nf], np.int32)


def brute_force(lp):
    """(ends, total) by enumeration, for lp whose sums are exact in float64 (small integers, dyadic fractions): the maximal total,
    and among the paths that reach it the one the tie rule selects.  Walking back from the last frame the rule stays on phoneme j
    whenever some optimal path stays, so it makes the start of the last phoneme as early as an optimal path allows, then the start
    of the one before it, ...: the minimum of (ends[nl-2], ends[nl-3], ..., ends[0]) in lexicographic order."""
    lp = np.asarray(lp, np.float64)
    nf, nl = lp.shape
    best = None
    for e in all_paths(nf, nl):
        key = (-path_sum(lp, e), tuple(int(v) for v in e[-2::-1]))
        if best is None or key < best[0]:
            best = (key, e)
    return best[1], -best[0][0]


def planted(nf, nl, heads, d, seed, margin=4.0):
    """q, k (float32 values exactly representable in fp16) whose alignment is known: k_j = 2 e_j in every head (needs nl <= d),
    q_t = 2 e_{path(t)}; with scale s the true phoneme's score leads every other by 4 s, so lp of the true path wins every row by
    more than 1 when 4 s >= margin.  Returns q, k, scale, ends."""
    assert nl <= d and nf >= nl
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, nf), nl - 1, replace=False)) if nl > 1 else np.array([], np.int64)
    ends = np.concatenate((cuts, [nf])).astype(np.int32)
    path = path_of(ends, nf)
    k = np.zeros((nl, heads * d), np.float32)
    q = np.zeros((nf, heads * d), np.float32)
    for h in range(heads):
        k[np.arange(nl), h * d + np.arange(nl)] = 2.0
        q[np.arange(nf), h * d + path] = 2.0
    return q, k, margin / 4.0, ends
