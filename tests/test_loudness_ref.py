"""CPU: the fp64 loudness mirror (tests/_loudness_ref.py) against ITU-R BS.1770, the product's coefficients against the mirror's,
and the request keys "loudness", "loudness_scope", "loudness_peak" (DESIGN.md section 4v)."""
import math

import numpy as np
import pytest
from scipy.signal import lfilter

import _loudness_ref as R


def test_mirror_coefficients_are_the_standards_at_48k():
    b1, a1, b2, a2 = R.k_coefficients(48000)
    got = np.concatenate([b1, a1[1:], a2[1:]])
    want = np.array(R.BS1770_48K["shelf_b"] + R.BS1770_48K["shelf_a"] + R.BS1770_48K["hp_a"])
    assert np.abs(got - want).max() <= 1e-12
    assert a1[0] == 1.0 and a2[0] == 1.0 and list(b2) == [1.0, -2.0, 1.0]


@pytest.mark.parametrize("rate", [24000, 32000, 48000])
def test_product_coefficients_equal_the_mirrors(rate):
    from gsv import audio_io
    k = audio_io.k_weighting(rate)
    b1, a1, b2, a2 = R.k_coefficients(rate)
    for got, want in zip(k["shelf"] + k["highpass"], (b1, a1, b2, a2)):
        assert np.abs(np.asarray(got) - want).max() <= 1e-15
    assert k["sub_block"] == int(round(0.1 * rate))
    assert audio_io.k_weighting(rate) is k                                  # cached per rate
    # the state-space form is the cascade: s' = A s + B x, y = C s + D x against lfilter
    x = np.random.default_rng(3).standard_normal(400)
    s, y = np.zeros(4), np.zeros(400)
    for i, v in enumerate(x):
        y[i] = k["C"] @ s + k["D"] * v
        s = k["A"] @ s + k["B"] * v
    assert np.abs(y - lfilter(b2, a2, lfilter(b1, a1, x))).max() <= 1e-12
    assert np.allclose(k["A4096"], np.linalg.matrix_power(k["A16"], 256), rtol=1e-9, atol=1e-300)
    assert audio_io.LOUDNESS_SCOPES == ("fragment", "sentence")


def test_full_scale_997_hz_sine_reads_minus_3_01():
    t = np.arange(2 * 48000) / 48000.0
    m = R.meter(np.sin(2 * np.pi * 997.0 * t), 48000)
    assert abs(m["lufs"] - (-3.01)) <= 0.01


def test_relative_gate_drops_the_quiet_blocks_and_keeps_the_straddling_ones():
    rate, s = 48000, 4800
    t = np.arange(2 * rate) / float(rate)
    x = np.sin(2 * np.pi * 997.0 * t)
    x[rate:] *= 10.0 ** (-25.0 / 20.0)
    m = R.meter(x, rate)
    assert abs(m["lufs"] - (-3.71)) <= 0.01
    assert m["abs"].all()
    nb = len(m["z"])                                                         # block b covers sub-blocks b .. b + 3; 10 are loud
    loud_part = np.array([max(0, min(10, b + 4) - b) for b in range(nb)])
    assert not m["rel"][loud_part == 0].any(), "a block of the quiet half alone was kept"
    assert m["rel"][loud_part >= 1].all(), "a block that holds loud samples was dropped"
    assert m["lufs"] > float(R.level(m["z"].mean()))                         # the ungated mean of all blocks reads lower


def test_absolute_gate_gives_minus_infinity_and_gain_one():
    t = np.arange(48000) / 48000.0
    x = np.sin(2 * np.pi * 997.0 * t) * 10.0 ** (-77.0 / 20.0)              # -80 LUFS
    m = R.meter(x, 48000)
    assert float(R.level(m["z"]).max()) < -70.0 and m["lufs"] == -math.inf
    g, flags = R.span_gain(m["lufs"], -20.0, 0.0, [x.astype(np.float32)])
    assert g == 1.0 and flags == R.SILENT


def test_short_span_rule():
    rate, s = 32000, 3200
    x = 0.25 * np.sin(2 * np.pi * 440.0 * np.arange(4 * s - 1) / rate)
    m = R.meter(x, rate)
    assert m["J"] == 3 and len(m["z"]) == 1 and len(m["energies"]) == 4
    assert m["z"][0] == pytest.approx(m["energies"].sum() / (4 * s - 1), rel=1e-12)
    assert math.isfinite(m["lufs"])
    assert len(R.meter(x[:0], rate)["z"]) == 0 and R.meter(x[:0], rate)["lufs"] == -math.inf
    assert len(R.meter(np.append(x, 0.0), rate)["z"]) == 1 and R.meter(np.append(x, 0.0), rate)["J"] == 4


def test_ceiling_and_limited_flag():
    x = (0.5 * np.sin(2 * np.pi * 997.0 * np.arange(48000) / 48000.0)).astype(np.float32)
    L = R.meter(x, 48000)["lufs"]
    g, flags = R.span_gain(L, L + 3.0, 0.0, [x])                              # +3 dB of 0.5 stays below full scale
    assert flags == 0 and g == pytest.approx(10.0 ** (3.0 / 20.0))
    g, flags = R.span_gain(L, L + 9.0, -1.0, [x])                             # +9 dB would reach 1.41
    P = float(np.abs(x).max())
    assert flags == R.LIMITED and g == pytest.approx(10.0 ** (-1.0 / 20.0) / P)
    assert R.span_gain(L, None, 0.0, [x]) == (1.0, 0)                         # meter only
    y = x.copy()
    y[5] = np.nan
    assert R.span_gain(L, -20.0, 0.0, [x, y]) == (1.0, R.NAN)
    loud = (x * 4.0).astype(np.float32)                                       # peak 2: normalised, P = 1
    assert R.norm_sentence(loud)[0].max() == pytest.approx(1.0)
    g, flags = R.span_gain(-10.0, -5.0, 0.0, [loud])
    assert flags == R.LIMITED and g == 1.0


# ---- the request keys ------------------------------------------------------------------------------------------------------------
def _options(req):
    from gsv.TTS_infer_pack.TTS import TTS
    return TTS._request_options(req)


def test_request_options_carry_the_keys_only_with_loudness():
    from gsv.TTS_infer_pack.TTS import TTS
    base = _options({"text": "a"})
    assert not any(k.startswith("loudness") for k in base)
    assert set(base) == {"top_k", "top_p", "temperature", "batch_size", "batch_threshold", "speed_factor", "split_bucket",
                         "return_fragment", "fragment_interval", "parallel_infer", "repetition_penalty", "sample_steps",
                         "inference_cfg_rate", "super_sampling", "seed"}          # the dict of a request before this feature
    assert TTS._format_kw(base) == {}
    o = _options({"loudness": -20})
    assert (o["loudness"], o["loudness_scope"], o["loudness_peak"]) == (-20.0, "fragment", 0.0)
    assert {k: v for k, v in o.items() if not k.startswith("loudness")} == base
    o = _options({"loudness": -16.5, "loudness_scope": "sentence", "loudness_peak": -1, "sample_rate": 8000, "encoding": "mulaw"})
    assert TTS._format_kw(o) == {"sample_rate": 8000, "encoding": "mulaw", "loudness": -16.5, "loudness_scope": "sentence",
                                 "loudness_peak": -1.0}
    assert _options({"loudness": None}) == base
    o = _options({"loudness": np.float32(-20.0), "loudness_peak": np.float64(-1.0)})     # any real number, as a float
    assert (o["loudness"], o["loudness_peak"]) == (-20.0, -1.0) and type(o["loudness"]) is float
    assert _options({"loudness": 0})["loudness"] == 0.0 and _options({"loudness": -70.0})["loudness"] == -70.0


@pytest.mark.parametrize("req", [{"loudness_scope": "sentence"}, {"loudness_peak": -1.0}, {"loudness": "-20"}, {"loudness": True}, {"loudness": np.bool_(True)},
                                 {"loudness": 0.5}, {"loudness": -70.5}, {"loudness": float("nan")},
                                 {"loudness": -20, "loudness_scope": "word"}, {"loudness": -20, "loudness_peak": 0.1},
                                 {"loudness": -20, "loudness_peak": "0"}, {"loudness": -20, "loudness_peak": float("nan")}])
def test_request_options_refuse(req):
    with pytest.raises(ValueError):
        _options(req)


@pytest.mark.parametrize("key, value", [("loudness", -20.0), ("loudness_scope", "sentence"), ("loudness_peak", -1.0)])
def test_sharded_runs_refuse_the_keys(key, value):
    from gsv import sharding
    sharding.refuse_output_format([{"text": "a"}, {}])
    with pytest.raises(ValueError, match=key):
        sharding.refuse_output_format([{"text": "a"}, {"text": "b", key: value}])
