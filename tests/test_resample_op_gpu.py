"""GPU: gsv_op_resample_poly_seg (csrc/resample.hip) against scipy.signal.resample_poly in fp64.

Error bar, per output (derived, not measured; tests/_resample_ref.py error_bar):
    |y - ref| <= (t_i + 2) 2^-24 S_i + 2^-24 |ref|,   S_i = sum |h x| over the output's t_i taps
-- fp32 accumulation of t_i products in any order with a filter rounded to fp32.  Inputs are uniform in +-1.5.

One call per rate pair with 5 segments of 1, 3, 37, 1501 samples and one whose output spans three whole workgroup tiles plus a
ragged tail (the kernel's tile is TILE = 1024 outputs: 3 * 1024 + 317), with gaps between the segments in both streams."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from _resample_ref import error_bar, out_len, resample_mirror, up_down

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 1024                        # csrc/resample.hip kRsTile
GSV_ERR_ARG = -1                   # include/gsv.h
SENTINEL = -77.25
PAIRS = [(32000, 16000), (48000, 16000), (44100, 16000), (44100, 32000), (16000, 32000)]


def _st():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _i32(v):
    return (C.c_int32 * max(1, len(v)))(*[int(a) for a in v])


def _call(x, h, up, down, in_start, in_len, out_start, y, peak, n_seg=None, n_x=None, n_y=None, h_len=None):
    from gsv import _lib
    _lib.init(0)
    rc = _lib.lib().gsv_op_resample_poly_seg(x.data_ptr(), x.numel() if n_x is None else n_x, h.data_ptr(), h.numel() if h_len is None else h_len,
                                             up, down, len(in_len) if n_seg is None else n_seg, _i32(in_start), _i32(in_len), _i32(out_start),
                                             y.data_ptr(), y.numel() if n_y is None else n_y, None if peak is None else peak.data_ptr(), _st())
    torch.cuda.synchronize()
    return rc


@functools.lru_cache(maxsize=None)
def _case(pair):
    """the segments of one rate pair, their fp64 references and bars, and the device results of ONE call (shared by the tests)"""
    from scipy.signal import resample_poly
    from gsv.audio_io import resample_filter
    up, down = up_down(*pair)
    h, u, d = resample_filter(*pair)
    assert (u, d) == (up, down)
    n_long = -(-(3 * TILE + 317) * down // up)
    lens = [1, 3, 37, 1501, n_long]
    assert out_len(n_long, up, down) >= 3 * TILE + 317 and out_len(n_long, up, down) % TILE != 0
    rng = np.random.default_rng(pair[0] + pair[1])
    xs = [rng.uniform(-1.5, 1.5, n).astype(np.float32) for n in lens]
    refs, bars = [], []
    for x in xs:
        ref = resample_poly(x.astype(np.float64), up, down)
        mir, S, taps = resample_mirror(x, h, up, down)            # the fp32 filter's own terms
        assert ref.shape == mir.shape
        refs.append(ref)
        bars.append(error_bar(ref, S, taps))
    ms = [r.shape[0] for r in refs]
    in_start, out_start, a, b = [], [], 5, 3                      # gaps of 5, 6, ... samples in front of the segments
    for s, (n, m) in enumerate(zip(lens, ms)):
        in_start.append(a)
        out_start.append(b)
        a += n + 5 + s
        b += m + 2 + s
    stream = np.full(a, 1e6, dtype=np.float32)                    # what lies between the segments must never enter
    for x, o in zip(xs, in_start):
        stream[o:o + x.shape[0]] = x
    xd, hd = torch.from_numpy(stream).to(DEV), torch.from_numpy(h).to(DEV)
    y = torch.full((b,), SENTINEL, dtype=torch.float32, device=DEV)
    peak = torch.full((len(lens),), float("nan"), dtype=torch.float32, device=DEV)
    rc = _call(xd, hd, up, down, in_start, lens, out_start, y, peak)
    return dict(up=up, down=down, h=hd, xs=xs, lens=lens, ms=ms, refs=refs, bars=bars, in_start=in_start, out_start=out_start, x=xd,
                y=y, peak=peak, rc=rc)


@pytest.mark.parametrize("pair", PAIRS)
def test_within_the_fp32_error_bar_of_scipy(pair):
    c = _case(pair)
    assert c["rc"] == 0
    y = c["y"].cpu().numpy().astype(np.float64)
    worst = 0.0
    for s, (o, m) in enumerate(zip(c["out_start"], c["ms"])):
        err = np.abs(y[o:o + m] - c["refs"][s])
        bar = c["bars"][s]
        assert np.all(bar > 0)
        worst = max(worst, float((err / bar).max()))
    print(f"{pair}: worst |y - ref| / bar = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("pair", PAIRS)
def test_untouched_samples_and_peak(pair):
    c = _case(pair)
    assert c["rc"] == 0
    y = c["y"].cpu()
    inside = torch.zeros(y.numel(), dtype=torch.bool)
    for s, (o, m) in enumerate(zip(c["out_start"], c["ms"])):
        inside[o:o + m] = True
        assert c["peak"][s].item() == y[o:o + m].abs().max().item()                 # exactly: a maximum has no rounding
    assert inside.sum().item() < y.numel() and torch.all(y[~inside] == SENTINEL)
    assert not torch.any(y[inside] == SENTINEL)


@pytest.mark.parametrize("pair", PAIRS)
def test_position_independence(pair):
    """the same segments in reversed order, at other offsets and with other neighbours: torch.equal per segment"""
    c = _case(pair)
    order = list(range(len(c["lens"])))[::-1]
    in_start, out_start, a, b = {}, {}, 0, 1029                                      # the outputs shifted by more than a tile
    for s in order:
        in_start[s], out_start[s] = a, b
        a += c["lens"][s] + 1
        b += c["ms"][s] + 7
    stream = np.full(a, -3e5, dtype=np.float32)
    for s in order:
        stream[in_start[s]:in_start[s] + c["lens"][s]] = c["xs"][s]
    y = torch.full((b,), SENTINEL, dtype=torch.float32, device=DEV)
    peak = torch.empty(len(order), dtype=torch.float32, device=DEV)
    rc = _call(torch.from_numpy(stream).to(DEV), c["h"], c["up"], c["down"], [in_start[s] for s in order], [c["lens"][s] for s in order],
               [out_start[s] for s in order], y, peak)
    assert rc == 0
    for k, s in enumerate(order):
        want = c["y"][c["out_start"][s]:c["out_start"][s] + c["ms"][s]]
        assert torch.equal(y[out_start[s]:out_start[s] + c["ms"][s]], want), f"segment {s}"
        assert peak[k].item() == c["peak"][s].item()
    # one segment alone, without a peak array
    s = 3
    y1 = torch.empty(c["ms"][s], dtype=torch.float32, device=DEV)
    assert _call(torch.from_numpy(c["xs"][s]).to(DEV), c["h"], c["up"], c["down"], [0], [c["lens"][s]], [0], y1, None) == 0
    assert torch.equal(y1, c["y"][c["out_start"][s]:c["out_start"][s] + c["ms"][s]])


def test_argument_errors_return_before_any_launch():
    """argument checks only: every call is refused on the host, and y keeps its sentinel"""
    c = _case((44100, 16000))
    up, down, h, x = c["up"], c["down"], c["h"], c["x"]
    lens, ins, outs = c["lens"], c["in_start"], c["out_start"]
    y = torch.full((c["y"].numel(),), SENTINEL, dtype=torch.float32, device=DEV)
    peak = torch.full((len(lens),), SENTINEL, dtype=torch.float32, device=DEV)
    big = torch.zeros(8193, dtype=torch.int32).tolist()
    bad = [
        dict(n_seg=0), dict(n_seg=8193, in_start=big, in_len=big, out_start=big),
        dict(in_len=[1, 0, 37, 1501, lens[4]]), dict(in_len=[1, 3, -5, 1501, lens[4]]),
        dict(up=0), dict(down=0), dict(up=-1),
        dict(h_len=h.numel() - 1),                                                     # even
        dict(h_len=65537),                                                             # odd, but above the cap (never read)
        dict(up=1, down=1000, h_len=21),                                               # window of a tile above the kernel's LDS
        dict(in_start=[ins[0], ins[1], ins[1] + 2, ins[3], ins[4]]),                   # overlapping inputs
        dict(in_start=[ins[1], ins[0]] + ins[2:]),                                     # descending inputs
        dict(out_start=[outs[0], outs[1], outs[1] + 1, outs[3], outs[4]]),             # overlapping outputs
        dict(out_start=outs[:3] + [outs[4], outs[3]]),                                 # descending outputs
        dict(n_x=ins[4] + lens[4] - 1),                                                # the last input range leaves the stream
        dict(n_y=outs[4] + c["ms"][4] - 1),                                            # the last output range leaves y
        dict(in_start=[-1] + ins[1:]), dict(out_start=[-1] + outs[1:]),
    ]
    for kw in bad:
        a = dict(up=up, down=down, in_start=ins, in_len=lens, out_start=outs)
        a.update(kw)
        rc = _call(x, h, a.pop("up"), a.pop("down"), a.pop("in_start"), a.pop("in_len"), a.pop("out_start"), y, peak, **a)
        assert rc == GSV_ERR_ARG, kw
        assert torch.all(y == SENTINEL) and torch.all(peak == SENTINEL), kw
    from gsv import _lib
    assert b"op_resample_poly_seg" in _lib.lib().gsv_last_error()
    assert _call(x, h, up, down, ins, lens, outs, y, peak) == 0                        # and the good call still runs
    assert torch.equal(y, c["y"])
