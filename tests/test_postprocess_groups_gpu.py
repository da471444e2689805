"""GPU: `gsv_postprocess_groups` (csrc/sola.hip) -- the fragments of a whole server step in one launch pair -- must write, for
every group, bit for bit what `gsv_postprocess` writes when it is called for that group alone with the group's gap.  The
sentences are views at odd element offsets into larger buffers (what torch.split hands the pipeline), so neither the sources
nor the destinations are 16-byte aligned in general."""
import ctypes as C

import numpy as np
import pytest
import torch

from gsv import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

LENGTHS = [0, 1, 7, 8, 9, 1023, 1025, 4099]


def _sentence(g, n, kind, dt):
    x = torch.rand(n, generator=g) * 1.6 - 0.8                  # |x| < 0.8: no division
    if n == 0:
        return x.to(dt)
    if kind == "one":
        x[int(n // 2)] = -1.0                                   # peak exactly 1.0: no division
    elif kind == "loud":
        x = x * 4.0
        x[n - 1] = 3.25                                         # peak above 1: divided
    elif kind == "nan":
        x = x * 4.0
        x[int(n // 3)] = float("nan")                           # a NaN anywhere: no division
    elif kind == "zero":
        x.zero_()
    return x.to(dt)


def _views(sentences, dt):
    """each sentence as a view into one device buffer, sentence i starting 1 + i % 7 elements past a 16-byte boundary"""
    per = 16 // torch.empty(0, dtype=dt).element_size()
    starts, at = [], 0
    for i, s in enumerate(sentences):
        at = (at + per - 1) // per * per + 1 + i % 7
        starts.append(at)
        at += int(s.numel())
    buf = torch.zeros(at + per, dtype=dt, device=DEV)
    assert buf.data_ptr() % 16 == 0
    out = []
    for s, a in zip(sentences, starts):
        buf[a:a + s.numel()] = s.to(DEV)
        out.append(buf[a:a + s.numel()])
        assert s.numel() == 0 or (out[-1].data_ptr() % 16) // s.element_size() == a % per
    return buf, out


def _one_by_one(views, gap, code):
    """gsv_postprocess for one group: the yardstick"""
    n = len(views)
    lens = [int(v.numel()) for v in views]
    pcm = torch.full((sum(lens) + gap * n + 1,), 0x5a5a, dtype=torch.int16, device=DEV)
    ptrs = (C.c_void_p * max(n, 1))(*[v.data_ptr() for v in views])
    arr = (C.c_int * max(n, 1))(*lens)
    st = torch.cuda.current_stream()
    _lib.check(_lib.lib().gsv_postprocess(ptrs, arr, n, code, gap, pcm.data_ptr(), C.c_void_p(st.cuda_stream)), "gsv_postprocess")
    torch.cuda.synchronize()
    return pcm[:-1].cpu().numpy()


def _grouped(groups, code):
    """gsv_postprocess_groups over [(views, gap)] -> (packed int16 with one guard sample on either side, offsets)"""
    flat = [v for views, _ in groups for v in views]
    n = len(flat)
    lens = (C.c_int * max(n, 1))(*[int(v.numel()) for v in flat])
    ptrs = (C.c_void_p * max(n, 1))(*[v.data_ptr() for v in flat])
    gn = (C.c_int * max(len(groups), 1))(*[len(v) for v, _ in groups])
    gg = (C.c_int * max(len(groups), 1))(*[g for _, g in groups])
    off = (C.c_longlong * (len(groups) + 1))()
    l = _lib.lib()
    need = int(l.gsv_postprocess_groups_workspace(lens, n))
    assert need >= 0
    table = torch.empty(max(need, 16), dtype=torch.uint8).pin_memory()
    work = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
    total = sum(int(v.numel()) + g for views, g in groups for v in views)
    pcm = torch.full((total + 2,), 0x5a5a, dtype=torch.int16, device=DEV)     # [1:-1] is the output: an odd byte offset / 2
    st = torch.cuda.current_stream()
    _lib.check(l.gsv_postprocess_groups(ptrs, lens, n, code, gn, gg, len(groups), pcm.data_ptr() + 2, off, table.data_ptr(),
                                        work.data_ptr(), C.c_void_p(st.cuda_stream)), "gsv_postprocess_groups")
    torch.cuda.synchronize()
    return pcm.cpu().numpy(), [int(o) for o in off]


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_groups_equal_one_call_per_group(half):
    dt, code = (torch.float16, _lib.GSV_F16) if half else (torch.float32, _lib.GSV_F32)
    g = torch.Generator().manual_seed(11)
    kinds = ["plain", "one", "loud", "nan", "zero"]
    groups_host = []
    # every length with every kind, spread over groups of differing size with gaps 0 and 3 (odd: the destinations that follow
    # start at odd sample offsets); lengths 1023 / 1025 / 4099 straddle the vector body and the 4096-sample tile
    cases = [(n, k) for k in kinds for n in LENGTHS]
    sizes, at = [1, 3, 2, 5, 4, 7, 6, 12], 0
    for gi, sz in enumerate(sizes):
        groups_host.append(([_sentence(g, n, k, dt) for n, k in cases[at:at + sz]], 3 if gi % 2 == 0 else 0))
        at += sz
    assert at == len(cases) == 40
    # one group of 40 sentences: past the 32 entries of gsv_postprocess's by-value table
    groups_host.append(([_sentence(g, [9, 1025, 7, 130][i % 4], kinds[i % 5], dt) for i in range(40)], 3))
    # a group without sentences, and one long sentence of several tiles at gap 0
    groups_host.append(([], 3))
    groups_host.append(([_sentence(g, 3 * 4096 + 5, "loud", dt)], 0))
    keep, groups = [], []
    for sentences, gap in groups_host:
        buf, views = _views(sentences, dt)
        keep.append(buf)
        groups.append((views, gap))
    packed, off = _grouped(groups, code)
    assert off[0] == 0 and off[-1] == len(packed) - 2
    assert packed[0] == 0x5a5a and packed[-1] == 0x5a5a, "a sample outside the packed buffer was written"
    packed = packed[1:-1]
    for gi, (views, gap) in enumerate(groups):
        want = _one_by_one(views, gap, code)
        got = packed[off[gi]:off[gi + 1]]
        assert off[gi + 1] - off[gi] == len(want) == sum(int(v.numel()) + gap for v in views)
        assert np.array_equal(got, want), f"group {gi} ({len(views)} sentences, gap {gap}): {int((got != want).sum())} samples differ"
    # the sentences are what their kinds say (in the dtype under test): a peak of exactly 1, a peak above 1, a NaN
    for n in LENGTHS[1:]:
        assert float(_sentence(g, n, "one", dt).abs().max()) == 1.0 and float(_sentence(g, n, "loud", dt).abs().max()) > 1.0
        assert bool(torch.isnan(_sentence(g, n, "nan", dt)).any()) and float(_sentence(g, n, "plain", dt).abs().max()) < 1.0
    # and the division shows in the output: the loud sentence's last sample is its peak, 3.25 -> 1.0 -> -32768 after the wrap
    (views, _), o = groups[-1], off[-2]
    assert packed[o + views[0].numel() - 1] == -32768


def test_no_sentence_is_ok_and_bad_arguments_are_refused():
    l = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    off = (C.c_longlong * 3)(7, 7, 7)
    gn, gg = (C.c_int * 2)(0, 0), (C.c_int * 2)(3, 0)
    assert l.gsv_postprocess_groups(None, None, 0, _lib.GSV_F32, None, None, 0, None, None, None, None, st) == 0
    assert l.gsv_postprocess_groups(None, None, 0, _lib.GSV_F16, gn, gg, 2, None, off, None, None, st) == 0
    assert list(off) == [0, 0, 0]
    assert l.gsv_postprocess_groups_workspace(None, 0) == 0
    assert l.gsv_postprocess_groups_workspace((C.c_int * 2)(4, -1), 2) == -1
    x = torch.zeros(8, device=DEV)
    ptrs, lens = (C.c_void_p * 1)(x.data_ptr()), (C.c_int * 1)(8)
    work = torch.empty(64, dtype=torch.uint8, device=DEV)
    table = torch.empty(64, dtype=torch.uint8)
    pcm = torch.zeros(16, dtype=torch.int16, device=DEV)
    bad_n = (C.c_int * 1)(2)            # the groups name two sentences, n is one
    assert l.gsv_postprocess_groups(ptrs, lens, 1, _lib.GSV_F32, bad_n, gg, 1, pcm.data_ptr(), off, table.data_ptr(), work.data_ptr(), st) == -1
    assert l.gsv_postprocess_groups(ptrs, lens, 1, 7, (C.c_int * 1)(1), gg, 1, pcm.data_ptr(), off, table.data_ptr(), work.data_ptr(), st) == -1
    torch.cuda.synchronize()


def test_pipeline_wrapper_returns_what_audio_postprocess_returns_per_fragment():
    """TTS.postprocess_fragments against audio_postprocess([frags], sr, None, speed, False, interval), fragment by fragment"""
    from gsv.TTS_infer_pack.TTS import TTS
    for half in (False, True):
        tts = TTS({"device": DEV, "is_half": half, "version": "v2"})
        dt = torch.float16 if half else torch.float32
        g = torch.Generator().manual_seed(29)
        frags = []
        for i, (lens, interval) in enumerate([([700, 1, 5000], 0.3), ([4099], 0.01), ([33, 0, 64, 129], 0.05)]):
            wav = (torch.rand(sum(lens), generator=g) * (3.0 if i != 1 else 1.0) - 0.5).to(DEV, dt)
            frags.append((list(torch.split(wav, lens)), interval))
        got = tts.postprocess_fragments(frags)
        for (fr, interval), a in zip(frags, got):
            sr, want = tts.audio_postprocess([fr], 32000, None, 1.0, False, interval, False)
            assert a.dtype == np.int16 and np.array_equal(a, want)
        assert tts.postprocess_fragments([]) == []
