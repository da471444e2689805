"""GPU: gsv_op_frame_seg is gsv_op_frame per segment, bit for bit, in f32 and f16: the STFT framing of the reference
spectrogram (n_fft 2048, hop 640, reflect padding 704), plain strided frames (10 / 5 / 0) and an operand wider than the frame
(ld > frame_len).  The segments include one of pad + 1 samples, the shortest legal one, and rows between the segments keep what
they held."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GSV_ERR_ARG = -1
SENTINEL = -3.5
# (frame_len, hop, pad, ld, segment lengths)
CASES = [(2048, 640, 704, 2048, [705, 3200, 2048, 9001]),
         (10, 5, 0, 10, [1 + 9, 37, 10, 643]),
         (10, 5, 0, 16, [12, 1501]),
         (400, 100, 150, 512, [151, 977, 400])]


def _st():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _i32(v):
    return (C.c_int32 * max(1, len(v)))(*[int(a) for a in v])


def _frames(n, flen, hop, pad):
    return max(1, (n + 2 * pad - flen) // hop + 1) if n + 2 * pad >= flen else 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("case", CASES)
def test_bit_equal_to_op_frame_per_segment(case, dtype):
    from gsv import _lib
    _lib.init(0)
    l = _lib.lib()
    flen, hop, pad, ld, lens = case
    g = torch.Generator().manual_seed(flen + ld)
    xs = [torch.rand(n, generator=g) * 2 - 1 for n in lens]
    Ts = [_frames(n, flen, hop, pad) for n in lens]
    if (flen, pad) == (2048, 704):
        assert lens[0] == pad + 1 and Ts[0] == 1                       # 705 + 1408 = 2113 samples: exactly one frame
    assert all(t >= 1 for t in Ts)
    x_start, row_start, a, r = [], [], 3, 2
    for s, (n, t) in enumerate(zip(lens, Ts)):
        x_start.append(a)
        row_start.append(r)
        a += n + 4
        r += t + (1 if s % 2 == 0 else 0)                               # a gap row behind every other segment
    stream = torch.full((a,), 1e4)
    for x, o in zip(xs, x_start):
        stream[o:o + x.numel()] = x
    stream = stream.to(DEV)
    out = torch.full((r + 1, ld), SENTINEL, dtype=dtype, device=DEV)
    rc = l.gsv_op_frame_seg(stream.data_ptr(), stream.numel(), flen, hop, pad, ld, len(lens), _i32(x_start), _i32(lens), _i32(row_start),
                            _i32(Ts), out.shape[0], out.data_ptr(), _lib.dtype_code(dtype), _st())
    assert rc == 0, l.gsv_last_error()
    inside = torch.zeros(out.shape[0], dtype=torch.bool)
    for x, t, r0 in zip(xs, Ts, row_start):
        xd = x.to(DEV)
        want = torch.full((t, ld), SENTINEL, dtype=dtype, device=DEV)
        _lib.check(l.gsv_op_frame(xd.data_ptr(), x.numel(), flen, hop, pad, ld, t, want.data_ptr(), _lib.dtype_code(dtype), _st()), "gsv_op_frame")
        torch.cuda.synchronize()
        assert torch.equal(out[r0:r0 + t], want)
        assert torch.all(want[:, flen:] == 0)
        inside[r0:r0 + t] = True
    assert (~inside).sum() >= 3 and torch.all(out[~inside.to(DEV)] == SENTINEL)


def test_argument_errors():
    from gsv import _lib
    _lib.init(0)
    l = _lib.lib()
    x = torch.zeros(4000, device=DEV)
    out = torch.full((8, 2048), SENTINEL, device=DEV)

    def call(x_start, x_len, row_start, row_len, n_seg=None, pad=704, rows=8, n_x=4000, dtype=0):
        rc = l.gsv_op_frame_seg(x.data_ptr(), n_x, 2048, 640, pad, 2048, len(x_len) if n_seg is None else n_seg, _i32(x_start), _i32(x_len),
                                _i32(row_start), _i32(row_len), rows, out.data_ptr(), dtype, _st())
        torch.cuda.synchronize()
        return rc

    assert call([0], [704], [0], [1]) == GSV_ERR_ARG                     # not longer than the reflect padding
    assert call([0], [705], [0], [2]) == GSV_ERR_ARG                     # frames past the padded signal
    assert call([0, 700], [705, 705], [0, 1], [1, 1]) == GSV_ERR_ARG     # overlapping samples
    assert call([0, 1000], [705, 705], [1, 1], [1, 1]) == GSV_ERR_ARG    # overlapping rows
    assert call([0, 3500], [705, 705], [0, 1], [1, 1]) == GSV_ERR_ARG    # past the stream
    assert call([0], [705], [8], [1]) == GSV_ERR_ARG                     # past the operand
    assert call([0], [705], [0], [1], n_seg=0) == GSV_ERR_ARG
    assert call([0], [705], [0], [1], dtype=7) == GSV_ERR_ARG
    assert torch.all(out == SENTINEL)
    assert call([0, 1000], [705, 705], [0, 1], [1, 1]) == 0
