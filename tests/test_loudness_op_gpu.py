"""GPU: `gsv_op_loudness` (csrc/sola.hip), the device meter of gsv_postprocess_groups_loud, against the
sequential fp64 mirror of tests/_loudness_ref.py.

Bars (from the issue that introduced the meter, not from what the kernels give):
* every sub-block energy above the absolute-gate level within 1e-9 relative: fp64 rounding times the filter's noise gain and a
  sum over <= 4800 terms give about 1e-12, the chunked order measured 1.4e-12 in emulation; 1e-9 stays five orders below what an
  off-by-one chunk, tile or sub-block border produces;
* |L - L_mirror| <= 1e-8 LU (4.34 x the energy bar); the fp32 gain within 1 ulp of float32(mirror gain); equal flags.
No block of a metered span may lie within 0.01 LU of a gate in the mirror (asserted): the seeds are chosen so."""
import math

import numpy as np
import pytest

import _loudness_gpu as G
import _loudness_ref as R

pytestmark = pytest.mark.gpu
RATES = [24000, 32000, 48000]
DTYPES = [np.float16, np.float32]
WORST = {"energy": 0.0, "lufs": 0.0}


def _lengths(rate):
    s = int(round(0.1 * rate))
    return [0, 1, 15, 16, 17, 4095, 4096, 4097, 8193, 12293, 4 * s - 1, 4 * s, 4 * s + 1, 5 * s, 90001]


def length_case(dt, rate, seed=11):
    """one sentence-scope span per length, each sentence the only one of its group"""
    rng = np.random.default_rng(seed)
    groups, spans = [], []
    for i, n in enumerate(_lengths(rate)):
        groups.append(([G.speech(rng, n, rate).astype(dt)], 5))
        spans.append((i, 1, False, (-23.0, -16.0, None)[i % 3], (0.0, -1.0)[i % 2]))
    return groups, spans


def fragment_case(dt, rate, seed=23):
    """fragment-scope spans over groups of many short sentences, and the gate cases"""
    rng = np.random.default_rng(seed)

    def sentences(k, amp=0.3):
        return [G.speech(rng, int(rng.integers(300, 701)), rate, amp).astype(dt) for _ in range(k)]

    a = sentences(40)                                   # gap 7: an empty sentence and one with peak 1.7 (it is normalised)
    a[9] = a[9][:0]
    a[17] = (a[17].astype(np.float64) / np.abs(a[17].astype(np.float64)).max() * 1.7).astype(dt)
    b = sentences(40)                                   # gap 0
    c = sentences(6)                                    # gap 0.3 R
    d = sentences(5)                                    # a NaN: gain 1
    d[2] = d[2].copy()
    d[2][100] = np.nan
    n = int(0.7 * rate)                                 # loud, then 25 dB down
    e = G.speech(rng, 2 * n, rate)
    e[n:] *= 10.0 ** (-25.0 / 20.0)
    f = G.speech(rng, int(0.5 * rate), rate) * 10.0 ** (-61.0 / 20.0)     # about -80 LUFS: below the absolute gate
    z = np.zeros(int(0.5 * rate))
    h = sentences(12)                                   # gap 7 in the stream, left out of the span: sentences 2 .. 9 without gaps
    groups = [(a, 7), (b, 0), (c, int(0.3 * rate)), (d, 7), ([e.astype(dt)], 0), ([f.astype(dt)], 0), ([z.astype(dt)], 0), (h, 7)]
    spans, first = [], 0
    for i, (sents, _) in enumerate(groups[:-1]):
        spans.append((first, len(sents), True, (-23.0, -16.0, None)[i % 3], (0.0, -1.0)[i % 2]))
        first += len(sents)
    spans.append((first + 2, 8, False, -18.0, 0.0))
    return groups, spans


def _run(groups, spans, rate):
    energies, rep = G.op_loudness(groups, spans, rate)
    for k, span in enumerate(spans):
        m, g, flags = G.mirror_span(groups, span, rate)
        if not flags & R.NAN:
            assert R.gate_margin(m) >= 0.01, (k, R.gate_margin(m))
        G.check_span(energies[k], rep[k], m, g, flags, WORST)
    print("worst fraction of the energy bar %.3g, of the level bar %.3g" % (WORST["energy"], WORST["lufs"]))
    return rep


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "fp32"])
def test_span_lengths(dt, rate):
    """0 .. 17 samples, the tile borders, the short-span rule around 4 s, and 90 001 samples: a 22-tile carry chain, a sub-block
    longer than a tile at 48 kHz and two sub-block borders inside a tile at 24 kHz"""
    groups, spans = length_case(dt, rate)
    rep = _run(groups, spans, rate)
    assert int(rep[0]["flags"]) == R.SILENT and float(rep[0]["lufs"]) == -math.inf          # the empty span
    assert math.isfinite(float(rep[1]["lufs"]))                                              # one sample still gets a level


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("dt", DTYPES, ids=["fp16", "fp32"])
def test_fragment_scope(dt, rate):
    """streams that cross sentence and gap borders inside chunks and tiles, misaligned sources, a normalised and an empty
    sentence, a NaN, the relative gate (loud then -25 dB), the absolute gate (-80 LUFS), silence, and a span of several
    sentences without their gaps"""
    groups, spans = fragment_case(dt, rate)
    rep = _run(groups, spans, rate)
    assert int(rep[3]["flags"]) & R.NAN and float(rep[3]["gain"]) == 1.0
    m, _, _ = G.mirror_span(groups, spans[4], rate)
    assert m["abs"].all() and not m["rel"].all() and m["rel"].any()                          # the relative gate drops blocks
    assert int(rep[5]["flags"]) == R.SILENT and int(rep[6]["flags"]) == R.SILENT
