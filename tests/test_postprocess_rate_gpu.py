"""GPU: `gsv_postprocess_groups_rate` (csrc/sola.hip) -- the groups of `gsv_postprocess_groups` at another
sample rate and in another encoding.  Per group the kernel resamples the virtual stream concat_i [norm(x_i), gap zeros] (what
`gsv_postprocess_f32` writes for that group alone) with the polyphase FIR of `gsv_op_resample_poly_seg` and converts:

* the identity filter with F32 output is that stream, which pins norm;
* F32 output lies within the derived bar of tests/_resample_ref.py (`error_bar`) of the fp64 mirror of that stream;
* S16 is y * 32768 in fp32, clamped and truncated, of the kernel's own F32 output, and saturates where the FIR overshoots;
* MULAW / ALAW are the bytes of Python's audioop for every int16 value;
* a group's bits do not depend on the launch it is part of.

The sentences are views at odd element offsets (what torch.split hands the pipeline)."""
import ctypes as C

import numpy as np
import pytest
import torch

from _resample_ref import error_bar, out_len, resample_mirror, up_down
from gsv import _lib, audio_io

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

PAIRS = [(32000, 8000), (32000, 44100), (32000, 22050), (32000, 11025), (24000, 16000), (48000, 44100)]
OUT_DT = {_lib.GSV_OUT_S16: torch.int16, _lib.GSV_OUT_MULAW: torch.uint8, _lib.GSV_OUT_ALAW: torch.uint8,
          _lib.GSV_OUT_F32: torch.float32}
# (sentence lengths with their peaks, gap).  Group 0: peak 1.7 next to peak 0.4 with a sentence of 7 and gaps of 3 between them,
# so one FIR window spans sentence -> gap -> sentence -> gap -> sentence and the scale changes inside it; group 1: gaps of 9600
# samples (tile borders fall inside a gap) around an empty sentence; group 2 has no sentence; group 3: gap 0, a border inside a
# sentence; group 4: one empty sentence without a gap (no sample at all); group 5: 1 sample, then a long sentence.
GROUPS = [([(5000, 1.7), (7, 0.9), (4097, 0.4)], 3), ([(1023, 0.8), (0, 0.0), (1, 1.0)], 9600), ([], 3),
          ([(4097, 1.7), (1023, 0.4)], 0), ([(0, 0.0)], 0), ([(1, 0.5), (5000, 2.5)], 3)]


def _sentence(g, n, peak, dt):
    x = torch.rand(n, generator=g) * 2.0 - 1.0
    if n:
        x = x / x.abs().max() * peak
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
    out = []
    for s, a in zip(sentences, starts):
        buf[a:a + s.numel()] = s.to(DEV)
        out.append(buf[a:a + s.numel()])
    return buf, out


def _groups(dt, seed=5, spec=GROUPS):
    g = torch.Generator().manual_seed(seed)
    keep, groups = [], []
    for sents, gap in spec:
        buf, views = _views([_sentence(g, n, pk, dt) for n, pk in sents], dt)
        keep.append(buf)
        groups.append((views, gap))
    return keep, groups


def _stream(views, gap):
    """gsv_postprocess_f32 of one group: the fp32 stream the kernel resamples"""
    n = len(views)
    lens = [int(v.numel()) for v in views]
    wav = torch.full((sum(lens) + gap * n + 1,), 7.0, dtype=torch.float32, device=DEV)
    if n:
        ptrs = (C.c_void_p * n)(*[v.data_ptr() for v in views])
        st = torch.cuda.current_stream()
        _lib.check(_lib.lib().gsv_postprocess_f32(ptrs, (C.c_int * n)(*lens), n, _lib.dtype_code(views[0].dtype), gap, wav.data_ptr(),
                                                  C.c_void_p(st.cuda_stream)), "gsv_postprocess_f32")
    torch.cuda.synchronize()
    return wav[:-1].cpu().numpy()


def _rate(groups, code, h, up, down, fmt, shift=1):
    """gsv_postprocess_groups_rate over [(views, gap)] -> (one array per group, offsets); the output starts `shift` elements
    past a 16-byte boundary and has a guard element on either side"""
    flat = [v for views, _ in groups for v in views]
    n = len(flat)
    lens = (C.c_int * max(n, 1))(*[int(v.numel()) for v in flat])
    ptrs = (C.c_void_p * max(n, 1))(*[v.data_ptr() for v in flat])
    gn = (C.c_int * max(len(groups), 1))(*[len(v) for v, _ in groups])
    gg = (C.c_int * max(len(groups), 1))(*[g for _, g in groups])
    off = (C.c_longlong * (len(groups) + 1))()
    l = _lib.lib()
    need = int(l.gsv_postprocess_groups_rate_workspace(lens, n, len(groups)))
    assert need >= 0
    table = torch.empty(max(need, 16), dtype=torch.uint8).pin_memory()
    work = torch.empty(max(need, 16), dtype=torch.uint8, device=DEV)
    total = sum(out_len(sum(int(v.numel()) + g for v in views), up, down) for views, g in groups)
    guard = 0x5a if OUT_DT[fmt] != torch.float32 else 1234.5
    out = torch.full((total + shift + 1,), guard, dtype=OUT_DT[fmt], device=DEV)
    hd = torch.from_numpy(np.ascontiguousarray(h, dtype=np.float32)).to(DEV)
    st = torch.cuda.current_stream()
    _lib.check(l.gsv_postprocess_groups_rate(ptrs, lens, n, code, gn, gg, len(groups), out.data_ptr() + shift * out.element_size(), off,
                                             table.data_ptr(), work.data_ptr(), hd.data_ptr(), int(hd.numel()), up, down, fmt,
                                             C.c_void_p(st.cuda_stream)), "gsv_postprocess_groups_rate")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    off = [int(o) for o in off]
    assert off[0] == 0 and off[-1] == total
    assert (got[:shift] == guard).all() and got[-1] == guard, "an element outside the packed buffer was written"
    got = got[shift:-1]
    return [got[off[g]:off[g + 1]] for g in range(len(groups))], off


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _s16(y):
    """the stated conversion on the host: y * 32768 in fp32, clamped to [-32768, 32767], truncated toward zero"""
    q = np.clip(y.astype(np.float32) * np.float32(32768.0), np.float32(-32768.0), np.float32(32767.0))
    return np.trunc(q).astype(np.int16)


# ---- G.711 on the host: audioop where Python still has it, else the numpy restatement below (pinned on the corner values)
def _g711_numpy(pcm, law):
    v = pcm.astype(np.int32)
    if law == "mulaw":
        v = v >> 2
        mask = np.where(v < 0, 0x7f, 0xff)
        v = np.minimum(np.abs(v), 8159) + 33
        seg = np.searchsorted(np.array([0x3f, 0x7f, 0xff, 0x1ff, 0x3ff, 0x7ff, 0xfff, 0x1fff]), v, side="left")
        code = np.where(seg >= 8, 0x7f, (seg << 4) | ((v >> (np.minimum(seg, 7) + 1)) & 0xf))
        return (code ^ mask).astype(np.uint8)
    v = v >> 3
    mask = np.where(v < 0, 0x55, 0xd5)
    v = np.where(v < 0, -v - 1, v)
    seg = np.searchsorted(np.array([0x1f, 0x3f, 0x7f, 0xff, 0x1ff, 0x3ff, 0x7ff, 0xfff]), v, side="left")
    code = (seg << 4) | ((v >> np.where(seg < 2, 1, seg)) & 0xf)
    return (code ^ mask).astype(np.uint8)


def _g711(pcm, law):
    pcm = np.ascontiguousarray(pcm, dtype="<i2")
    try:
        import audioop
    except ImportError:
        for k, u, a in ((0, 0xff, 0xd5), (32767, 0x80, 0xaa), (-32768, 0x00, 0x2a)):
            one = np.array([k], dtype=np.int16)
            assert int(_g711_numpy(one, "mulaw")[0]) == u and int(_g711_numpy(one, "alaw")[0]) == a
        return _g711_numpy(pcm, law)
    fn = audioop.lin2ulaw if law == "mulaw" else audioop.lin2alaw
    return np.frombuffer(fn(pcm.tobytes(), 2), dtype=np.uint8)


FMT_OF = {"mulaw": _lib.GSV_OUT_MULAW, "alaw": _lib.GSV_OUT_ALAW}


@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_identity_filter_is_the_normalised_stream(half):
    dt = torch.float16 if half else torch.float32
    keep, groups = _groups(dt)
    got, _ = _rate(groups, _lib.dtype_code(dt), [1.0], 1, 1, _lib.GSV_OUT_F32)
    for gi, (views, gap) in enumerate(groups):
        want = _stream(views, gap)
        assert got[gi].shape == want.shape
        # fmaf(1, x, +0) is x for every x but -0: the values are compared, and the bits wherever the stream is not zero
        assert np.array_equal(got[gi], want), f"group {gi}"
        nz = want != 0
        assert _same_bits(got[gi][nz], want[nz]), f"group {gi}"
    assert float(np.abs(got[0][:5000]).max()) == 1.0 and float(np.abs(got[5][4:]).max()) == 1.0     # the loud sentences are divided
    assert abs(float(np.abs(got[0][5013:]).max()) - 0.4) < 1e-3                                       # the quiet one is not


@pytest.fixture(scope="module")
def f32_runs():
    """per (dtype, pair): the kernel's F32 output per group and the fp64 mirror of each group's stream -- computed once"""
    cache = {}

    def get(half, pair):
        if (half, pair) not in cache:
            dt = torch.float16 if half else torch.float32
            keep, groups = _groups(dt)
            h, up, down = audio_io.resample_filter(*pair)
            assert (up, down) == up_down(*pair)
            got, off = _rate(groups, _lib.dtype_code(dt), h, up, down, _lib.GSV_OUT_F32)
            refs = [resample_mirror(_stream(views, gap), h, up, down) for views, gap in groups]
            cache[(half, pair)] = (keep, groups, got, refs, (h, up, down))
        return cache[(half, pair)]
    return get


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
def test_f32_output_within_the_derived_bar_of_the_fp64_mirror(f32_runs, half, pair):
    _, groups, got, refs, (h, up, down) = f32_runs(half, pair)
    hlds = max(1024, (1023 * down + len(h) - 1) // up + 2) + len(h) <= 16384
    assert hlds == (pair not in [(32000, 11025), (48000, 11025)])        # 32000 -> 11025 reads its filter through L2
    worst = 0.0
    for gi, ((views, gap), (ref, S, taps)) in enumerate(zip(groups, refs)):
        assert got[gi].shape == ref.shape == (out_len(sum(int(v.numel()) + gap for v in views), up, down),)
        err, bar = np.abs(got[gi].astype(np.float64) - ref), error_bar(ref, S, taps)
        if len(ref):
            worst = max(worst, float((err / np.maximum(bar, 1e-300)).max()) if (bar > 0).any() else 0.0)
        assert (err <= bar).all(), f"group {gi}: {int((err > bar).sum())} outputs beyond the bar, worst ratio {float((err / np.maximum(bar, 1e-300)).max()):.3f}"
    print(f"\n{pair[0]} -> {pair[1]} {'f16' if half else 'f32'}: worst |err| / bar = {worst:.3f}")
    assert len(got[2]) == 0 and len(got[4]) == 0                         # no sentence, and no sample


@pytest.mark.parametrize("pair", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_s16_is_the_stated_conversion_and_saturates(pair):
    h, up, down = audio_io.resample_filter(*pair)
    n = 4000
    sq = torch.where((torch.arange(n) // 40) % 2 == 0, 1.0, -1.0)        # +-1, period 80: the FIR overshoots its peak
    keep, views = _views([sq.to(torch.float32)], torch.float32)
    groups = [(views, 3)]
    ref, _, _ = resample_mirror(_stream(views, 3), h, up, down)
    assert ref.max() > 1.0 and ref.min() < -1.0, "the mirror does not overshoot: the case checks nothing"
    y = _rate(groups, _lib.GSV_F32, h, up, down, _lib.GSV_OUT_F32)[0][0]
    q = _rate(groups, _lib.GSV_F32, h, up, down, _lib.GSV_OUT_S16)[0][0]
    assert q.dtype == np.int16 and np.array_equal(q, _s16(y))
    over, under = y * np.float32(32768.0) >= 32767.0, y * np.float32(32768.0) <= -32768.0
    assert over.any() and under.any()
    assert (q[over] == 32767).all() and (q[under] == -32768).all(), "an overshoot wrapped"
    # and on random groups, f16 input, an odd output address
    keep2, g2 = _groups(torch.float16)
    ys, _ = _rate(g2, _lib.GSV_F16, h, up, down, _lib.GSV_OUT_F32, shift=3)
    qs, _ = _rate(g2, _lib.GSV_F16, h, up, down, _lib.GSV_OUT_S16, shift=3)
    for a, b in zip(ys, qs):
        assert np.array_equal(b, _s16(a))


@pytest.mark.parametrize("law", ["mulaw", "alaw"])
def test_g711_of_every_int16_value(law):
    k = torch.arange(-32768, 32768, dtype=torch.float32) / 32768.0      # exact in fp32; the identity filter hands k on
    keep, views = _views([k], torch.float32)
    got = _rate([(views, 0)], _lib.GSV_F32, [1.0], 1, 1, FMT_OF[law], shift=5)[0][0]
    pcm = _rate([(views, 0)], _lib.GSV_F32, [1.0], 1, 1, _lib.GSV_OUT_S16)[0][0]
    assert np.array_equal(pcm, np.arange(-32768, 32768).astype(np.int16))
    want = _g711(pcm, law)
    assert got.dtype == np.uint8 and np.array_equal(got, want), f"{int((got != want).sum())} codes differ"


@pytest.mark.parametrize("law", ["mulaw", "alaw"])
def test_g711_of_a_resampled_group(law):
    h, up, down = audio_io.resample_filter(32000, 8000)
    keep, groups = _groups(torch.float16)
    pcm, off = _rate(groups, _lib.GSV_F16, h, up, down, _lib.GSV_OUT_S16)
    got, off2 = _rate(groups, _lib.GSV_F16, h, up, down, FMT_OF[law], shift=7)
    assert off == off2
    for a, b in zip(pcm, got):
        assert np.array_equal(b, _g711(a, law))


@pytest.mark.parametrize("pair", [(32000, 44100), (32000, 11025)], ids=["lds-filter", "l2-filter"])
def test_a_group_does_not_depend_on_its_launch(pair):
    h, up, down = audio_io.resample_filter(*pair)
    keep, groups = _groups(torch.float16)
    assert len(groups) == 6
    together, _ = _rate(groups, _lib.GSV_F16, h, up, down, _lib.GSV_OUT_F32)
    order = [3, 5, 0, 4, 1, 2]
    moved, _ = _rate([groups[i] for i in order], _lib.GSV_F16, h, up, down, _lib.GSV_OUT_F32, shift=2)
    for gi, grp in enumerate(groups):
        alone, _ = _rate([grp], _lib.GSV_F16, h, up, down, _lib.GSV_OUT_F32, shift=3)
        assert _same_bits(alone[0], together[gi]), f"group {gi} alone"
        assert _same_bits(moved[order.index(gi)], together[gi]), f"group {gi} at another position"
    # a NaN sentence in group 3 changes no other group
    keep2, bad = _groups(torch.float16)
    bad[3][0][1][100] = float("nan")
    poisoned, _ = _rate(bad, _lib.GSV_F16, h, up, down, _lib.GSV_OUT_F32)
    for gi in (0, 1, 2, 4, 5):
        assert _same_bits(poisoned[gi], together[gi]), f"group {gi} next to a NaN"
    assert np.isnan(poisoned[3]).any()
    for fmt in (_lib.GSV_OUT_S16, _lib.GSV_OUT_MULAW, _lib.GSV_OUT_ALAW):    # the conversions take a NaN without a fault
        _rate(bad, _lib.GSV_F16, h, up, down, fmt)


def test_empty_calls_and_refused_arguments():
    l = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    off = (C.c_longlong * 3)(7, 7, 7)
    gn, gg = (C.c_int * 2)(0, 0), (C.c_int * 2)(3, 0)
    hd = torch.ones(1, device=DEV)
    assert l.gsv_postprocess_groups_rate(None, None, 0, _lib.GSV_F16, gn, gg, 2, None, off, None, None, hd.data_ptr(), 1, 1, 1,
                                         _lib.GSV_OUT_S16, st) == 0
    assert list(off) == [0, 0, 0]
    assert l.gsv_postprocess_groups_rate_workspace(None, 0, 0) == 0
    assert l.gsv_postprocess_groups_rate_workspace((C.c_int * 2)(4, -1), 2, 1) == -1
    x = torch.zeros(8, device=DEV)
    ptrs, lens, one = (C.c_void_p * 1)(x.data_ptr()), (C.c_int * 1)(8), (C.c_int * 1)(1)
    work = torch.empty(256, dtype=torch.uint8, device=DEV)
    table = torch.empty(256, dtype=torch.uint8)
    out = torch.zeros(64, dtype=torch.float32, device=DEV)

    def call(h_len=1, up=1, down=1, fmt=_lib.GSV_OUT_S16):
        return l.gsv_postprocess_groups_rate(ptrs, lens, 1, _lib.GSV_F32, one, gg, 1, out.data_ptr(), off, table.data_ptr(),
                                             work.data_ptr(), hd.data_ptr(), h_len, up, down, fmt, st)
    assert call(fmt=9) == -1 and b"out_fmt" in l.gsv_last_error()
    assert call(h_len=2) == -1 and call(up=0) == -1 and call(h_len=65537) == -1
    assert call(h_len=20 * 640 + 1, up=1, down=640) == -1 and b"window" in l.gsv_last_error()       # 32000 -> 50
    assert call() == 0
    torch.cuda.synchronize()
