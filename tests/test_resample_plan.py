"""CPU: the host side of the device front-end.  The fp64 polyphase mirror of tests/_resample_ref.py is
scipy.signal.resample_poly (1e-12; below 1e-15 here) on seven rate pairs at lengths 1, 3, 37 and 700..2207; audio_io.resample_filter
is the filter resample_poly designs; output lengths and the grouping by input rate; and the two new entries are declared,
listed and exported."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from _resample_ref import RATE_PAIRS, out_len, resample_mirror, up_down

LENGTHS = [1, 3, 37, 700, 1501, 2207]


def _x(n, seed):
    return np.random.default_rng(seed).uniform(-1.5, 1.5, n)


@pytest.mark.parametrize("pair", RATE_PAIRS)
def test_mirror_is_resample_poly(pair):
    from scipy.signal import resample_poly
    from gsv.audio_io import resample_filter
    up, down = up_down(*pair)
    h32, u, d = resample_filter(*pair)
    assert (u, d) == (up, down) and h32.dtype == np.float32 and h32.shape == (20 * max(up, down) + 1,)
    from scipy.signal import firwin
    h = firwin(20 * max(up, down) + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up       # the fp64 filter
    assert np.array_equal(h.astype(np.float32), h32)
    worst = 0.0
    for k, n in enumerate(LENGTHS):
        x = _x(n, 100 * k + up)
        want = resample_poly(x, up, down)
        got, S, taps = resample_mirror(x, h, up, down)
        assert got.shape == want.shape == (out_len(n, up, down),)
        assert taps.max() <= -(-h.shape[0] // up) and np.all(S >= np.abs(got) - 1e-12)
        worst = max(worst, float(np.abs(got - want).max()))
        # the filter handed in as `window` is taken as it is: resample_filter is what the default call designs
        assert np.array_equal(resample_poly(x, up, down, window=h / up), want)
    print(f"{pair}: mirror vs resample_poly max abs {worst:.3e}")
    assert worst <= 1e-12


def test_resample_filter_is_cached_and_resample_unchanged():
    from scipy.signal import resample_poly
    from gsv import audio_io as A
    assert A.resample_filter(44100, 16000)[0] is A.resample_filter(44100, 16000)[0]
    x = _x(1000, 7).astype(np.float32)
    assert np.array_equal(A.resample(x, 44100, 16000), resample_poly(x.astype(np.float64), 160, 441).astype(np.float32))
    assert A.resample(x, 16000, 16000) is x


def test_lengths_and_grouping():
    from gsv import audio_io as A
    for sr_in, sr_out in RATE_PAIRS:
        for n in LENGTHS + [96000, 264600]:
            assert A.resampled_len(n, sr_in, sr_out) == A.resample(np.zeros(n, np.float32), sr_in, sr_out).shape[0] == -(-n * sr_out // sr_in)
    assert A.resampled_len(5, 16000, 16000) == 5
    assert A.group_by_rate([32000, 44100, 32000, 16000, 44100]) == {32000: [0, 2], 44100: [1, 4], 16000: [3]}
    assert list(A.group_by_rate([32000, 44100, 32000])) == [32000, 44100]                         # first appearance
    # every pair of the usual rates is inside the kernel's caps (include/gsv.h), 44.1 <-> 32 kHz and 22.05 -> 32 kHz among them
    rates = [16000, 22050, 24000, 32000, 44100, 48000]
    assert all(A.device_resample_supported(a, b) for a in rates for b in rates if a != b)
    assert len(A.resample_filter(44100, 32000)[0]) == len(A.resample_filter(32000, 44100)[0]) == 8821
    assert len(A.resample_filter(22050, 32000)[0]) == 12801
    assert not A.device_resample_supported(48000, 1000)                                           # window of 1024 outputs > 16384 samples
    assert not A.device_resample_supported(44100, 48001)                                          # filter of 960021 taps


def test_new_entries_are_declared_and_exported():
    from gsv import _lib
    src = open(os.path.join(ROOT, "include", "gsv.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = ("gsv_op_resample_poly_seg", "gsv_op_frame_seg")
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in include/gsv.h"
        assert name in _lib.EXPORTS
    assert re.search(r"int gsv_abi_version\(void\) \{ return 1; \}", open(os.path.join(ROOT, "gpt-sovits_amd", "csrc", "ops.hip")).read())
    from gsv import build
    assert os.path.join(build.CSRC, "resample.hip") in build.sources()
    build.build(verbose=False)
    l = _lib.lib()
    assert all(hasattr(l, name) for name in names) and l.gsv_abi_version() == 1
