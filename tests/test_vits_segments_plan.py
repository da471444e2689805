"""CPU: the layout of the segmented SoVITS decode (gsv_vits_segment_gap / gsv_vits_segment_map, host-only entry points of
the library that gsv_vits_decode_segments plans with): the gap between segments and the segment id of every row at
each resolution, checked against the rule written out independently here."""
import ctypes as C
import math

import numpy as np

from gsv import build, synthetic as S


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


def _gap_rule(model):
    """smallest G (frames) such that G * prod(rates[:i]) covers the one-sided reach of every conv reading resolution i"""
    need = [(model["kernel_size"] - 1) // 2, 2, 3]            # encoder FFN, WN in_layers (kernel 5), conv_pre (kernel 7)
    cum = 1
    for u, k in zip(model["upsample_rates"], model["upsample_kernel_sizes"]):
        p = (k - u) // 2
        need.append(math.ceil(max(math.ceil((k - 1 - p) / u), (u - 1 + p) // u) / cum))
        cum *= u
        for kk, ds in zip(model["resblock_kernel_sizes"], model["resblock_dilation_sizes"]):
            need += [math.ceil((kk - 1) // 2 * d / cum) for d in ds]
    need.append(math.ceil(3 / cum))                            # conv_post
    return max(1, max(need))


def _gap(lib, model):
    return lib.lib().gsv_vits_segment_gap(C.byref(_vc(lib, model)))


def test_gap_v2_config():
    lib = _lib()
    m = S.VITS_V2_CONFIG["model"]
    # frames: conv_pre reaches 3; after ups[0] (x10) ResBlock kernel 11 at dilation 5 reaches 25 rows = 3 frames
    assert _gap(lib, m) == 3 == _gap_rule(m)


def test_gap_other_configs():
    lib = _lib()
    small = S.small_vits_config()["model"]                     # rates [4, 2, 2]: 25 rows at x4 -> 7 frames
    assert _gap(lib, small) == 7 == _gap_rule(small)
    m = dict(S.VITS_V2_CONFIG["model"], upsample_rates=[2, 2], upsample_kernel_sizes=[4, 4], resblock_kernel_sizes=[11],
             resblock_dilation_sizes=[[1, 3, 7]])
    assert _gap(lib, m) == 18 == _gap_rule(m)                  # 5 * 7 = 35 rows at x2
    m = dict(S.VITS_V2_CONFIG["model"], upsample_rates=[8, 8, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4],
             resblock_kernel_sizes=[3, 5], resblock_dilation_sizes=[[1, 2, 3], [1, 2, 3]])
    assert _gap(lib, m) == 3 == _gap_rule(m)                   # conv_pre bounds it


def _map(lib, model, code_lens, phone_lens, level):
    vc = _vc(lib, model)
    n = len(code_lens)
    cl, pl = (C.c_int * n)(*code_lens), (C.c_int * n)(*phone_lens)
    rows = C.c_int64(0)
    assert lib.lib().gsv_vits_segment_map(C.byref(vc), n, cl, pl, level, None, 0, C.byref(rows)) == 0
    buf = (C.c_int32 * rows.value)()
    assert lib.lib().gsv_vits_segment_map(C.byref(vc), n, cl, pl, level, buf, rows.value, C.byref(rows)) == 0
    return np.frombuffer(buf, dtype=np.int32).copy()


def test_segment_maps_at_every_resolution():
    lib = _lib()
    m = S.VITS_V2_CONFIG["model"]
    G = _gap(lib, m)
    code_lens, phone_lens = [1, 7, 37], [3, 11, 2]
    # frames: 2 T_s rows per segment, G gap rows between neighbours, none at the ends
    want = np.concatenate([np.full(2, 0), np.full(G, -1), np.full(14, 1), np.full(G, -1), np.full(74, 2)]).astype(np.int32)
    assert np.array_equal(_map(lib, m, code_lens, phone_lens, 0), want)
    up = 1
    for i, u in enumerate(m["upsample_rates"]):
        up *= u
        assert np.array_equal(_map(lib, m, code_lens, phone_lens, i + 1), np.repeat(want, up)), f"stage {i}"
    # phones: the same gap between phone runs
    wl = np.concatenate([np.full(3, 0), np.full(G, -1), np.full(11, 1), np.full(G, -1), np.full(2, 2)]).astype(np.int32)
    assert np.array_equal(_map(lib, m, code_lens, phone_lens, -1), wl)
    # one segment: exactly the plain layout, no gap rows
    assert np.array_equal(_map(lib, m, [9], [4], 0), np.zeros(18, np.int32))


def test_packing_and_unpacking_offsets():
    """segment s starts at frame sum_{r<s} (2 T_r + G); its waveform starts at sample 2 sum_{r<s} T_r * prod(rates) once the
    gaps are dropped, so start - s * G * prod(rates) at the sample rate"""
    lib = _lib()
    m = S.small_vits_config()["model"]
    G = _gap(lib, m)
    code_lens, phone_lens = [5, 1, 12, 3], [2, 2, 9, 1]
    up = math.prod(m["upsample_rates"])
    sm = _map(lib, m, code_lens, phone_lens, len(m["upsample_rates"]))
    for s in range(len(code_lens)):
        rows = np.nonzero(sm == s)[0]
        start = sum(2 * t + G for t in code_lens[:s]) * up
        assert rows[0] == start and len(rows) == 2 * code_lens[s] * up and np.all(np.diff(rows) == 1)
        assert start - s * G * up == 2 * sum(code_lens[:s]) * up
    assert len(sm) == (2 * sum(code_lens) + 3 * G) * up


def test_bad_plans_are_rejected():
    lib = _lib()
    vc = _vc(lib, S.VITS_V2_CONFIG["model"])
    rows = C.c_int64(0)
    l = lib.lib()
    assert l.gsv_vits_segment_map(C.byref(vc), 2, (C.c_int * 2)(3, 0), (C.c_int * 2)(1, 1), 0, None, 0, C.byref(rows)) != 0
    assert b"empty" in l.gsv_last_error()
    assert l.gsv_vits_segment_map(C.byref(vc), 1, (C.c_int * 1)(3), (C.c_int * 1)(1), 9, None, 0, C.byref(rows)) != 0
