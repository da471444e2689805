"""CPU: the post layout of the segmented SoVITS decode with per-segment speeds (gsv_vits_segment_map_speed, host-only).
After the speed interpolation segment s has F_s frames (2 T_s at speed 1, int(2 T_s / speed) + 1 otherwise, as `decode`
counts them); the gap and the phone axis are those of the speed-1 layout."""
import ctypes as C
import math
import os
import re

import numpy as np

from gsv import build, synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the six segments of tests/test_vits_segments_speed_gpu.py
CODE_LENS = [1, 1, 6, 37, 11, 5]
PHONE_LENS = [3, 11, 23, 40, 9, 17]
SPEEDS = [0.5, 3.0, 1.5, 1.0, 1.3, 0.8]
FRAMES = [5, 1, 9, 74, 17, 13]


def _lib():
    from gsv import _lib
    build.build(verbose=False)
    return _lib


def _vc(lib, model):
    vc = lib.VitsConfig()
    vc.kernel_size = model["kernel_size"]
    vc.n_ups = len(model["upsample_rates"])
    for i, (u, k) in enumerate(zip(model["upsample_rates"], model["upsample_kernel_sizes"])):
        vc.up_rates[i], vc.up_kernels[i] = u, k
    vc.n_resblocks = len(model["resblock_kernel_sizes"])
    for j, (k, ds) in enumerate(zip(model["resblock_kernel_sizes"], model["resblock_dilation_sizes"])):
        vc.rb_kernels[j] = k
        for c, d in enumerate(ds):
            vc.rb_dilations[j][c] = d
    return vc


def _map(lib, model, code_lens, phone_lens, level, speeds="plain"):
    vc = _vc(lib, model)
    n = len(code_lens)
    cl, pl = (C.c_int * n)(*code_lens), (C.c_int * n)(*phone_lens)
    rows = C.c_int64(0)
    if speeds == "plain":
        def call(buf, cap):
            return lib.lib().gsv_vits_segment_map(C.byref(vc), n, cl, pl, level, buf, cap, C.byref(rows))
    else:
        sp = None if speeds is None else (C.c_double * n)(*speeds)

        def call(buf, cap):
            return lib.lib().gsv_vits_segment_map_speed(C.byref(vc), n, cl, pl, sp, level, buf, cap, C.byref(rows))
    assert call(None, 0) == 0, lib.lib().gsv_last_error()
    buf = (C.c_int32 * rows.value)()
    assert call(buf, rows.value) == 0
    return np.frombuffer(buf, dtype=np.int32).copy()


def test_frame_counts_are_those_of_decode():
    assert [2 * t if s == 1 else int(2 * t / s) + 1 for t, s in zip(CODE_LENS, SPEEDS)] == FRAMES


def test_all_speeds_one_is_the_plain_map():
    lib = _lib()
    for model in (S.VITS_V2_CONFIG["model"], S.small_vits_config()["model"]):
        for level in range(-1, len(model["upsample_rates"]) + 1):
            want = _map(lib, model, CODE_LENS, PHONE_LENS, level)
            assert np.array_equal(_map(lib, model, CODE_LENS, PHONE_LENS, level, [1.0] * 6), want), level
            assert np.array_equal(_map(lib, model, CODE_LENS, PHONE_LENS, level, None), want), level


def test_post_layout_of_the_six_segments():
    lib = _lib()
    for model in (S.VITS_V2_CONFIG["model"], S.small_vits_config()["model"]):
        G = lib.lib().gsv_vits_segment_gap(C.byref(_vc(lib, model)))
        for level in range(0, len(model["upsample_rates"]) + 1):
            up = math.prod(model["upsample_rates"][:level])
            parts = []
            for s, f in enumerate(FRAMES):
                if s:
                    parts.append(np.full(G * up, -1))
                parts.append(np.full(f * up, s))
            want = np.concatenate(parts).astype(np.int32)
            assert np.array_equal(_map(lib, model, CODE_LENS, PHONE_LENS, level, SPEEDS), want), level
        # the phone axis does not know about speed
        assert np.array_equal(_map(lib, model, CODE_LENS, PHONE_LENS, -1, SPEEDS), _map(lib, model, CODE_LENS, PHONE_LENS, -1))


def test_bad_speeds_are_rejected():
    lib = _lib()
    l = lib.lib()
    vc = _vc(lib, S.VITS_V2_CONFIG["model"])
    rows = C.c_int64(0)
    cl, pl = (C.c_int * 2)(3, 4), (C.c_int * 2)(1, 1)
    for bad in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
        assert l.gsv_vits_segment_map_speed(C.byref(vc), 2, cl, pl, (C.c_double * 2)(1.0, bad), 0, None, 0, C.byref(rows)) != 0
        assert b"speed" in l.gsv_last_error()
    # a slow-down whose post layout passes the 2^24-row limit although its pre layout does not
    big = (C.c_int * 2)(1 << 20, 4)
    assert l.gsv_vits_segment_map_speed(C.byref(vc), 2, big, pl, None, 0, None, 0, C.byref(rows)) == 0
    assert l.gsv_vits_segment_map_speed(C.byref(vc), 2, big, pl, (C.c_double * 2)(0.1, 1.0), 0, None, 0, C.byref(rows)) != 0
    assert b"too long" in l.gsv_last_error()
    assert l.gsv_vits_segment_map_speed(C.byref(vc), 2, big, pl, (C.c_double * 2)(1e-300, 1.0), 0, None, 0, C.byref(rows)) != 0


def test_symbols_are_declared():
    from gsv import _lib
    src = open(os.path.join(ROOT, "include", "gsv.h")).read()
    for name in ("gsv_vits_decode_segments_speed", "gsv_vits_segment_map_speed"):
        assert re.search(r"^int " + name + r"\(", src, re.M), name
        assert name in _lib.EXPORTS
    assert _lib.lib().gsv_abi_version() == 1
