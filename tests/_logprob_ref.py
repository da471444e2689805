"""fp64 mirror of the taken token's log-probability (csrc/t2s_sample.h token_logprob) and the bar the
fp32 device value is held to.

The quantity, for raw fp32 logits x, the step's unmasked vocabulary Veff and the taken token t:

    logp = (x[t] - m) - log(S),   m = max(x[:Veff]),   S = sum_{v < Veff} exp(x[v] - m);   -inf for t outside [0, Veff)

The device computes it in fp32 with one wave per row: 17 values per lane summed in sequence, then a 6-level butterfly.  With
eps = 2**-23 (one ulp relative; a correctly rounded operation errs by eps / 2), no fast-math, and expf / logf at their
documented 1 ulp:

* d = fl(x[t] - m): one rounding, |error| <= eps/2 * |d|;
* S: every argument fl(x[v] - m) carries a rounding of eps/2 * |x[v] - m|, which the exponential turns into a relative error
  of the term; weighted by the terms' shares p_v = exp(x[v] - m) / S this is eps/2 * sum p_v (m - x[v]) = eps/2 * (H(p) - log S)
  <= eps/2 * log(Veff) < 3.5 eps for Veff <= 1025.  expf adds 1 eps per term, the 17 sequential and 6 tree additions of
  positive terms 23 * eps/2.  Together S is off by at most (3.5 + 1 + 11.5) eps = 16 eps, relative;
* log: a relative error r of S moves log S by r (absolute), logf adds 1 eps * |log S|;
* the final subtraction: eps/2 * (|d| + |log S|).

Sum: eps * (16 + |d| + 1.5 |log S|).  Since 1 <= S <= Veff, |log S| <= 6.94, so this is below the bar the tests use,

    BAR = 2**-23 * (32 + 2 |x[t] - m| + |log S|)

(0.5 |log S| <= 3.5 < 16 + |d|).  The fp64 mirror's own error is 2**-29 times smaller and is not counted.  Terms that underflow
in fp32 (x[v] - m < -87) are below 1e-38 against S >= 1.
"""
import numpy as np

EPS = 2.0 ** -23


def token_logprob_ref(x, veff, tok):
    """(logp, bar) in float64 for one row of raw logits x (any float array, read as it is), vocabulary veff, token tok"""
    if not 0 <= tok < veff:
        return -np.inf, 0.0
    x64 = np.asarray(x, dtype=np.float64)[:veff]
    m = x64.max()
    S = np.exp(x64 - m).sum()
    d = x64[tok] - m
    return d - np.log(S), EPS * (32.0 + 2.0 * abs(d) + abs(np.log(S)))


def check_row(got, x, veff, tok, what=""):
    """asserts the device value `got` against the mirror; returns |error| / bar (0 for an exact -inf)"""
    ref, bar = token_logprob_ref(x, veff, tok)
    if np.isneginf(ref):
        assert np.isneginf(got), f"{what}: token {tok} outside [0, {veff}) must give -inf, got {got}"
        return 0.0
    err = abs(float(got) - ref)
    assert err <= bar, f"{what}: logp {got!r}, fp64 mirror {ref!r}: |error| {err:.3e} > bar {bar:.3e}"
    return err / bar
