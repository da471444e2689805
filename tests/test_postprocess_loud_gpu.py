"""GPU: `gsv_postprocess_groups_loud` (csrc/sola.hip) -- gsv_postprocess_groups_rate with every span of
sentences metered after ITU-R BS.1770 and multiplied by one gain in front of the filter taps.

* F32 at the identity filter is g * X within 2^-22 relative per sample (two fp32 roundings of 2^-24, the gain's own rounding);
* S16 within 1 LSB of the mirror's; G.711 bytes are the G.711 of the call's own S16;
* resampled F32 within the derived fp32 bar of tests/_resample_ref.py, evaluated on the gained stream;
* without spans the bytes are those of gsv_postprocess_groups_rate; a group's report and bytes do not depend on what else the
  call holds, on where the group sits in it, or on the run; the ceiling holds; bad descriptors are refused before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import _loudness_gpu as G
import _loudness_ref as R
from _resample_ref import error_bar, resample_mirror
from gsv import _lib, audio_io
from test_postprocess_rate_gpu import _g711

pytestmark = pytest.mark.gpu
ONE = (np.ones(1, dtype=np.float32), 1, 1)
FORMATS = [_lib.GSV_OUT_S16, _lib.GSV_OUT_MULAW, _lib.GSV_OUT_ALAW, _lib.GSV_OUT_F32]


def _groups(dt, rate, seed=41):
    """five groups: fragment scope with a normalised sentence; sentence scope under a -1 dB ceiling; no span; meter only; a
    target far above the level, so the ceiling limits the gain"""
    rng = np.random.default_rng(seed)
    sp = lambda n, amp=0.3: G.speech(rng, n, rate, amp).astype(dt)          # noqa: E731
    a = [sp(2500), sp(7), sp(1800)]
    a[0] = (a[0].astype(np.float64) / np.abs(a[0].astype(np.float64)).max() * 1.7).astype(dt)
    groups = [(a, 3), ([sp(1500, 0.1), sp(2100, 0.5)], 40), ([sp(900)], 5), ([sp(3000, 0.2)], 0), ([sp(2600, 0.05), sp(700, 0.05)], 11)]
    spans = [(0, 3, True, -23.0, 0.0), (3, 1, False, -16.0, -1.0), (4, 1, False, -16.0, -1.0), (6, 1, True, None, 0.0),
             (7, 2, True, -3.0, -2.0)]
    return groups, spans


def _gained_streams(groups, spans, rep, dtype=np.float32):
    """per group the stream the write launch filters: X_g with every span's sentences multiplied by its reported gain, the
    product rounded to fp32 as the kernel stages it (dtype=np.float64: the exact product)"""
    gain = {}
    for (first, count, _, _, _), r in zip(spans, rep):
        for i in range(first, first + count):
            gain[i] = np.float32(r["gain"])
    out, i = [], 0
    for sents, gap in groups:
        parts = []
        for x in sents:
            parts += [(R.norm_sentence(x)[0].astype(dtype) * dtype(gain.get(i, 1.0))).astype(dtype), np.zeros(gap, dtype=dtype)]
            i += 1
        out.append(np.concatenate(parts) if parts else np.zeros(0, dtype=np.float32))
    return out


@pytest.mark.parametrize("dt", [np.float16, np.float32], ids=["fp16", "fp32"])
def test_identity_filter_formats(dt):
    rate = 32000
    groups, spans = _groups(dt, rate)
    f32, rep = G.loud(groups, spans, rate, *ONE, _lib.GSV_OUT_F32)
    mirror = [G.mirror_span(groups, sp, rate) for sp in spans]
    for r, (m, g, flags) in zip(rep, mirror):
        assert int(r["flags"]) == flags and abs(float(r["lufs"]) - m["lufs"]) <= 1e-8 and G.ulps32(r["gain"], np.float32(g)) <= 1
    assert int(rep[4]["flags"]) == R.LIMITED and float(rep[3]["gain"]) == 1.0 and float(rep[0]["gain"]) != 1.0
    for got, exact in zip(f32, _gained_streams(groups, spans, rep, np.float64)):
        assert np.all(np.abs(got.astype(np.float64) - exact) <= 2.0 ** -22 * np.abs(exact))
    s16, rep16 = G.loud(groups, spans, rate, *ONE, _lib.GSV_OUT_S16)
    assert rep16.tobytes() == rep.tobytes()
    gm = {i: g for (first, count, _, _, _), (_, g, _) in zip(spans, mirror) for i in range(first, first + count)}
    i = 0
    for got, (sents, gap) in zip(s16, groups):
        parts = []
        for x in sents:
            parts += [R.s16(R.norm_sentence(x)[0].astype(np.float64) * gm.get(i, 1.0)), np.zeros(gap, dtype=np.int16)]
            i += 1
        assert np.abs(got.astype(np.int32) - np.concatenate(parts).astype(np.int32)).max() <= 1
    for fmt, law in ((_lib.GSV_OUT_MULAW, "mulaw"), (_lib.GSV_OUT_ALAW, "alaw")):
        got, _ = G.loud(groups, spans, rate, *ONE, fmt)
        for a, b in zip(got, s16):
            assert np.array_equal(a, _g711(b, law))


@pytest.mark.parametrize("sr_in, sr_out", [(32000, 8000), (24000, 48000), (32000, 44100)])
def test_resampled_within_the_fp32_bar(sr_in, sr_out):
    groups, spans = _groups(np.float32, sr_in)
    h, up, down = audio_io.output_filter(sr_in, sr_out)
    got, rep = G.loud(groups, spans, sr_in, h, up, down, _lib.GSV_OUT_F32)
    worst = 0.0
    for y, x in zip(got, _gained_streams(groups, spans, rep)):
        ref, S, taps = resample_mirror(x, h, up, down)
        bar = error_bar(ref, S, taps)
        err = np.abs(y.astype(np.float64) - ref)
        assert np.all(err <= bar)
        worst = max(worst, float((err[bar > 0] / bar[bar > 0]).max()))
    print("worst fraction of the resampling bar %d -> %d: %.3f" % (sr_in, sr_out, worst))


@pytest.mark.parametrize("fmt", FORMATS)
def test_zero_spans_are_the_rate_call(fmt):
    groups, _ = _groups(np.float16, 32000)
    h, up, down = audio_io.output_filter(32000, 8000)
    a, _ = G.loud(groups, [], 32000, h, up, down, fmt)
    b, _ = G.loud(groups, [], 32000, h, up, down, fmt, entry="rate")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_a_groups_bits_do_not_depend_on_the_call():
    rate = 32000
    groups, spans = _groups(np.float16, rate)
    h, up, down = audio_io.output_filter(rate, 8000)
    full, rep = G.loud(groups, spans, rate, h, up, down, _lib.GSV_OUT_S16)
    again, rep2 = G.loud(groups, spans, rate, h, up, down, _lib.GSV_OUT_S16, shift=3)
    assert rep.tobytes() == rep2.tobytes() and all(a.tobytes() == b.tobytes() for a, b in zip(full, again))
    # group 0 alone, and as the last of five
    alone, rep_a = G.loud(groups[:1], spans[:1], rate, h, up, down, _lib.GSV_OUT_S16)
    assert alone[0].tobytes() == full[0].tobytes() and rep_a[0].tobytes() == rep[0].tobytes()
    order = [1, 2, 3, 4, 0]
    moved, first = [], 0
    for g in order:
        cnt = len(groups[g][0])
        old_first = sum(len(groups[k][0]) for k in range(g))
        moved += [(first + f - old_first, c, gaps, t, p) for f, c, gaps, t, p in spans if old_first <= f < old_first + cnt]
        first += cnt
    last, rep_l = G.loud([groups[g] for g in order], moved, rate, h, up, down, _lib.GSV_OUT_S16)
    assert last[4].tobytes() == full[0].tobytes() and rep_l[-1].tobytes() == rep[0].tobytes()
    assert last[3].tobytes() == full[4].tobytes() and rep_l[-2].tobytes() == rep[4].tobytes()


def test_ceiling():
    rate = 32000
    groups, spans = _groups(np.float32, rate)
    s16, rep = G.loud(groups, spans, rate, *ONE, _lib.GSV_OUT_S16)
    assert int(rep[4]["flags"]) & R.LIMITED
    c = 10.0 ** (-2.0 / 20.0)
    assert abs(int(np.abs(s16[4].astype(np.int32)).max()) - round(c * 32768)) <= 1


@pytest.mark.parametrize("scope", ["fragment", "sentence"])
def test_postprocess_sentences_is_the_call(scope):
    """audio_io.postprocess_sentences (the command-line tool's path): float sentences, one group, the spans of the scope"""
    rate = 32000
    groups, _ = _groups(np.float32, rate)
    sents, gap = groups[0]
    spans = [(0, 3, True, -23.0, -1.0)] if scope == "fragment" else [(i, 1, False, -23.0, -1.0) for i in range(3)]
    want, rep = G.loud([(sents, gap)], spans, rate, *ONE, _lib.GSV_OUT_S16)
    got, reports = audio_io.postprocess_sentences(sents, gap, rate, None, None, "cuda:0", -23.0, scope, -1.0)
    assert got.dtype == np.int16 and got.tobytes() == want[0].tobytes()
    assert [(r[0], r[1]) for r in reports] == [(float(r["lufs"]), float(r["gain"])) for r in rep]
    plain, none = audio_io.postprocess_sentences(sents, gap, rate)
    assert none == [] and plain.shape == got.shape and not np.array_equal(plain, got)


BAD = [("unsorted", [(3, 1, False, -20.0, 0.0), (0, 3, True, -20.0, 0.0)]),
       ("overlapping", [(0, 2, True, -20.0, 0.0), (1, 1, True, -20.0, 0.0)]),
       ("crossing a group", [(2, 2, True, -20.0, 0.0)]),
       ("peak_db > 0", [(0, 3, True, -20.0, 0.5)]),
       ("target > 0", [(0, 3, True, 0.5, 0.0)]),
       ("target < -70", [(0, 3, True, -71.0, 0.0)]),
       ("past the end", [(7, 3, True, -20.0, 0.0)]),
       ("empty", [(0, 0, True, -20.0, 0.0)])]


@pytest.mark.parametrize("what, spans", BAD, ids=[b[0] for b in BAD])
def test_bad_descriptors_are_refused_before_any_launch(what, spans):
    _refused(spans, 32000)


def test_bad_rate_is_refused():
    _refused([(0, 3, True, -20.0, 0.0)], 0)
    _refused([(0, 3, True, -20.0, 0.0)], -32000)


def _refused(spans, rate):
    groups, _ = _groups(np.float32, 32000)
    c = G.Call(groups, spans, rate, "cuda:0")
    total = sum(x.shape[0] + g for sents, g in groups for x in sents)
    out = torch.full((total,), 1234.5, dtype=torch.float32, device="cuda:0")
    c.report.fill_(0x5a)
    hd = torch.ones(1, dtype=torch.float32, device="cuda:0")
    st = torch.cuda.current_stream()
    rc = _lib.lib().gsv_postprocess_groups_loud(c.ptrs, c.lens, c.n, c.code, c.gn, c.gg, c.ng, out.data_ptr(), c.off, c.table.data_ptr(),
                                                c.work.data_ptr(), hd.data_ptr(), 1, 1, 1, _lib.GSV_OUT_F32, rate, c.spans, c.ns,
                                                c.report.data_ptr(), C.c_void_p(st.cuda_stream))
    torch.cuda.synchronize()
    assert rc != 0
    assert b"postprocess_groups_loud" in _lib.lib().gsv_last_error()
    assert bool((out == 1234.5).all()) and bool((c.report == 0x5a).all()), "a refused call launched"
