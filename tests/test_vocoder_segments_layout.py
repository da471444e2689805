"""CPU: the layout of gsv_vocoder_forward_segments -- the gap between neighbouring segments and the row maps at every
resolution -- through the host-only exports gsv_vocoder_segment_gap / gsv_vocoder_segment_map.  No compute is called here."""
import ctypes as C
import math
import os
import re

import pytest

from conftest import ROOT
from gsv import synthetic as S

FRAMES = [1, 2, 7, 16]
GSV_ERR_ARG = None      # any non-zero code: the library's error codes are all non-zero


def _lib():
    from gsv import build, _lib
    build.build(verbose=False)
    return _lib


def _cfg(d):
    """the gsv_vocoder_config _VocoderEngine builds from a config dict"""
    L = _lib()
    c = L.VocoderConfig()
    c.kind = 1 if d["kind"] == "bigvgan" else 0
    c.in_channels, c.upsample_initial_channel = 100, d["upsample_initial_channel"]
    c.n_ups = len(d["upsample_rates"])
    for i, (u, k) in enumerate(zip(d["upsample_rates"], d["upsample_kernel_sizes"])):
        c.up_rates[i], c.up_kernels[i] = u, k
    c.n_resblocks = len(d["resblock_kernel_sizes"])
    for j, (k, ds) in enumerate(zip(d["resblock_kernel_sizes"], d["resblock_dilation_sizes"])):
        c.rb_kernels[j] = k
        for q, dil in enumerate(ds):
            c.rb_dilations[j][q] = dil
    return c


def _gap_rule(d):
    """The rule of the SoVITS segmented decode restricted to a vocoder: the smallest G whose
    G * prod(rates[:i]) rows cover, at every resolution, the one-sided input reach of each conv reading it."""
    ceil_div = lambda a, b: -(-a // b)
    g, cum = max(1, (7 - 1) // 2), 1                                   # conv_pre
    for u, k in zip(d["upsample_rates"], d["upsample_kernel_sizes"]):
        p = (k - u) // 2
        g = max(g, ceil_div(max(ceil_div(k - 1 - p, u), (u - 1 + p) // u), cum))   # transposed conv, in input rows
        cum *= u
        for rk, dils in zip(d["resblock_kernel_sizes"], d["resblock_dilation_sizes"]):
            for dil in dils:
                g = max(g, ceil_div((rk - 1) // 2 * dil, cum))         # convs1; convs2 (dilation 1) is never more
    return max(g, ceil_div(3, cum))                                    # conv_post


CONFIGS = [("bigvgan_v2", S.BIGVGAN_V2_24K_CONFIG, 7), ("hifigan_v4", S.HIFIGAN_V4_CONFIG, 3),
           ("bigvgan_small", S.small_vocoder_config("bigvgan"), 7), ("hifigan_small", S.small_vocoder_config("hifigan"), 7)]


@pytest.mark.parametrize("name,d,literal", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_gap_is_the_rule_of_the_segmented_decode(name, d, literal):
    got = _lib().lib().gsv_vocoder_segment_gap(C.byref(_cfg(d)))
    assert got == _gap_rule(d) == literal


def test_gap_agrees_with_the_sovits_rule_on_a_shared_shape():
    """one function serves both engines: a SoVITS config whose encoder and flow convs reach no further than conv_pre gets
    the gap of the vocoder with the same generator shape"""
    L = _lib()
    for d in (S.small_vocoder_config("hifigan"), S.HIFIGAN_V4_CONFIG):
        v, c = _cfg(d), L.VitsConfig()
        c.kernel_size = 3
        c.upsample_initial_channel, c.n_ups, c.n_resblocks = v.upsample_initial_channel, v.n_ups, v.n_resblocks
        for i in range(8):
            c.up_rates[i], c.up_kernels[i] = v.up_rates[i], v.up_kernels[i]
        for j in range(4):
            c.rb_kernels[j] = v.rb_kernels[j]
            for q in range(3):
                c.rb_dilations[j][q] = v.rb_dilations[j][q]
        assert L.lib().gsv_vits_segment_gap(C.byref(c)) == L.lib().gsv_vocoder_segment_gap(C.byref(v))


def _map(L, cfg, frames, level, cap=None):
    n = len(frames)
    G = L.lib().gsv_vocoder_segment_gap(C.byref(cfg))
    up = math.prod(cfg.up_rates[i] for i in range(level))
    rows = (sum(frames) + (n - 1) * G) * up
    buf = (C.c_int32 * (rows + 3))(*([-7] * (rows + 3)))
    rc = L.lib().gsv_vocoder_segment_map(C.byref(cfg), n, (C.c_int * n)(*frames), level, buf, rows if cap is None else cap)
    return rc, list(buf), rows, G, up


@pytest.mark.parametrize("name,d,literal", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_maps_at_every_level(name, d, literal):
    L = _lib()
    cfg = _cfg(d)
    for level in range(cfg.n_ups + 1):
        rc, buf, rows, G, up = _map(L, cfg, FRAMES, level)
        assert rc == 0
        assert buf[rows:] == [-7] * 3, "wrote past (sum F + (n - 1) G) * prod(rates[:level]) rows"
        seg = buf[:rows]
        want = []
        for s, f in enumerate(FRAMES):
            want += ([-1] * (G * up) if s else []) + [s] * (f * up)
        assert seg == want
        ids = [v for v in seg if v >= 0]
        assert ids == sorted(ids), "segment ids are non-decreasing"
        assert [seg.count(s) for s in range(len(FRAMES))] == [f * up for f in FRAMES]
        assert seg.count(-1) == (len(FRAMES) - 1) * G * up
        # one segment: no gap anywhere
        rc, one, rows1, _, _ = _map(L, cfg, [5], level)
        assert rc == 0 and rows1 == 5 * up and one[:rows1] == [0] * rows1


def test_bad_arguments_are_error_codes():
    L = _lib()
    cfg = _cfg(S.small_vocoder_config("bigvgan"))
    l = L.lib()
    buf = (C.c_int32 * 4096)()
    ok = (C.c_int * 2)(3, 4)
    assert l.gsv_vocoder_segment_map(C.byref(cfg), 2, ok, 0, buf, 4096) == 0
    assert l.gsv_vocoder_segment_map(None, 2, ok, 0, buf, 4096) != 0
    assert l.gsv_vocoder_segment_map(C.byref(cfg), 2, None, 0, buf, 4096) != 0
    assert l.gsv_vocoder_segment_map(C.byref(cfg), 2, ok, 0, None, 4096) != 0
    assert l.gsv_vocoder_segment_map(C.byref(cfg), 0, ok, 0, buf, 4096) != 0
    assert l.gsv_vocoder_segment_map(C.byref(cfg), 4097, (C.c_int * 4097)(*([1] * 4097)), 0, buf, 4096) != 0
    assert l.gsv_vocoder_segment_map(C.byref(cfg), 2, (C.c_int * 2)(3, 0), 0, buf, 4096) != 0
    assert l.gsv_vocoder_segment_map(C.byref(cfg), 2, ok, -1, buf, 4096) != 0
    assert l.gsv_vocoder_segment_map(C.byref(cfg), 2, ok, cfg.n_ups + 1, buf, 4096) != 0
    assert l.gsv_vocoder_segment_map(C.byref(cfg), 2, ok, 0, buf, 13) != 0, "3 + 7 + 4 rows do not fit 13"
    # 2^24 rows or more at the output rate (x16 here): 2^20 frames in all, gap included
    big = (C.c_int * 2)((1 << 19), (1 << 19) - 7)
    assert l.gsv_vocoder_segment_map(C.byref(cfg), 2, big, 0, buf, 1 << 30) != 0
    assert b"2^24" in l.gsv_last_error()
    bad = _cfg(S.small_vocoder_config("bigvgan"))
    bad.n_ups = 0
    assert l.gsv_vocoder_segment_gap(C.byref(bad)) == -1 and l.gsv_vocoder_segment_gap(None) == -1


def test_header_declares_the_new_entries_and_the_abi_version_stays():
    L = _lib()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gsv.h")).read(), flags=re.S)
    for name in ("gsv_vocoder_forward_segments", "gsv_vocoder_segment_gap", "gsv_vocoder_segment_map", "gsv_op_aa_act_cl"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src) and name in L.EXPORTS and hasattr(L.lib(), name)
    assert L.lib().gsv_abi_version() == 1
