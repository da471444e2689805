"""GPU: gsv_op_zero_rows and gsv_op_time_mean_seg, the two segmented kernels of the packed speaker-embedding pass (DESIGN.md
section 4l), against a numpy fp64 mirror.  T = 40 rows of ld = 24 floats; segments (0, 1), (8, 9), (24, 16): one of a single
row and one that ends at T.  The mean's bound is the fp32 summation bound 4 * len * 2^-24 * max|x| (len - 1 additions in some
order plus one division, each within 2^-24 relative of a partial sum that never exceeds len * max|x|)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, LD = 40, 24
SEGS = [(0, 1), (8, 9), (24, 16)]
GSV_ERR_ARG = -1                  # include/gsv.h


def _st():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _i32(v):
    return (C.c_int32 * max(1, len(v)))(*v)


def _x(seed, rows=T, ld=LD):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, ld, generator=g) * 3.0 + 1.5).to(DEV)


def _zero(maps, rows, T_=None, ld=None, n_maps=None, host_rows=None):
    from gsv import _lib
    _lib.init(0)
    zm = _lib.ZeroMaps()
    for i, m in enumerate(maps):
        zm.p[i] = m.data_ptr()
    dev = torch.tensor(rows if rows else [0], dtype=torch.int32, device=DEV)
    host = rows if host_rows is None else host_rows
    rc = _lib.lib().gsv_op_zero_rows(C.byref(zm), len(maps) if n_maps is None else n_maps, maps[0].shape[0] if T_ is None else T_,
                                     maps[0].shape[1] if ld is None else ld, dev.data_ptr(), _i32(host), len(rows), _st())
    torch.cuda.synchronize()
    return rc


def _mean_seg(x, segs, T_=None, ld=None, out=None):
    from gsv import _lib
    _lib.init(0)
    out = torch.full((len(segs), x.shape[1] if ld is None else ld), float("nan"), device=DEV) if out is None else out
    rc = _lib.lib().gsv_op_time_mean_seg(x.data_ptr(), x.shape[0] if T_ is None else T_, x.shape[1] if ld is None else ld, len(segs),
                                         _i32([a for a, _ in segs]), _i32([n for _, n in segs]), out.data_ptr(), _st())
    torch.cuda.synchronize()
    return rc, out


def test_zero_rows_zeroes_exactly_the_listed_rows():
    inside = {r for a, n in SEGS for r in range(a, a + n)}
    gaps = [r for r in range(T) if r not in inside]
    for n_maps in (1, 4, 8):
        maps = [_x(10 + i) for i in range(n_maps)]
        keep = [m.clone() for m in maps]
        untouched = _x(99)
        keep_u = untouched.clone()
        assert _zero(maps, gaps) == 0
        for m, k in zip(maps, keep):
            o, kk = m.cpu().numpy(), k.cpu().numpy()
            assert np.all(o[gaps] == 0.0) and not np.signbit(o[gaps]).any()
            rest = sorted(inside)
            assert np.array_equal(o[rest].view(np.uint32), kk[rest].view(np.uint32))          # bit-unchanged
        assert torch.equal(untouched, keep_u)
    # a wider map with more than one workgroup's worth of pieces, first and last row
    big = _x(3, rows=5, ld=4 * 300)
    kb = big.clone()
    assert _zero([big], [0, 4]) == 0
    assert bool((big[[0, 4]] == 0).all()) and torch.equal(big[1:4], kb[1:4])
    # an empty list is a call that does nothing
    m = _x(5)
    k = m.clone()
    assert _zero([m], []) == 0 and torch.equal(m, k)


def test_zero_rows_argument_errors():
    m = _x(1)
    k = m.clone()
    assert _zero([m], [3, T]) == GSV_ERR_ARG                       # a row outside [0, T)
    assert _zero([m], [-1]) == GSV_ERR_ARG
    assert _zero([m], [3], ld=22) == GSV_ERR_ARG                   # ld not a multiple of 4 floats
    assert _zero([m], [3], n_maps=0) == GSV_ERR_ARG
    assert _zero([m], [3], n_maps=9) == GSV_ERR_ARG
    assert torch.equal(m, k)                                       # a refused call stores nothing


def test_time_mean_seg_matches_fp64_mirror():
    x = _x(7)
    rc, out = _mean_seg(x, SEGS)
    assert rc == 0
    o, x64 = out.cpu().numpy().astype(np.float64), x.cpu().numpy().astype(np.float64)
    for i, (a, n) in enumerate(SEGS):
        ref = x64[a:a + n].mean(0)
        bound = 4.0 * n * 2.0 ** -24 * np.abs(x64[a:a + n]).max()
        err = np.abs(o[i] - ref).max()
        print(f"[time_mean_seg] segment ({a}, {n}): max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    assert np.array_equal(out[0].cpu().numpy(), x[0].cpu().numpy())               # one row: its own values


def test_time_mean_seg_depends_on_its_own_rows_alone():
    x = _x(8)
    _, out = _mean_seg(x, SEGS)
    y = _x(9)
    for a, n in SEGS[1:]:
        y[a:a + n] = x[a:a + n]
    _, out2 = _mean_seg(y, SEGS[1:])                                # other rows outside, other segments in the call
    assert torch.equal(out[1:].view(torch.int32), out2.view(torch.int32))
    # the same rows at another place of another array
    z = _x(11, rows=64)
    z[40:56] = x[24:40]
    _, out3 = _mean_seg(z, [(3, 2), (40, 16)])
    assert torch.equal(out[2].view(torch.int32), out3[1].view(torch.int32))


@pytest.mark.parametrize("rows,ld", [(T, LD), (37, 4 * 70), (1, 8)])
def test_single_segment_gives_time_mean_bits(rows, ld):
    from gsv import _lib
    x = _x(12, rows=rows, ld=ld)
    ref = torch.empty(ld, device=DEV)
    _lib.check(_lib.lib().gsv_op_time_mean(x.data_ptr(), rows, ld, ref.data_ptr(), _st()), "gsv_op_time_mean")
    rc, out = _mean_seg(x, [(0, rows)])
    assert rc == 0 and torch.equal(out[0].view(torch.int32), ref.view(torch.int32))


def test_time_mean_seg_argument_errors():
    x = _x(13)
    assert _mean_seg(x, [(0, 0)])[0] == GSV_ERR_ARG                 # an empty segment
    assert _mean_seg(x, [(8, 9), (0, 1)])[0] == GSV_ERR_ARG         # descending
    assert _mean_seg(x, [(0, 9), (8, 4)])[0] == GSV_ERR_ARG         # overlapping
    assert _mean_seg(x, [(30, 11)])[0] == GSV_ERR_ARG               # ends past T
    assert _mean_seg(x, [(0, 4)], ld=22)[0] == GSV_ERR_ARG          # ld not a multiple of 4
    assert _mean_seg(x, [])[0] == GSV_ERR_ARG                       # no segment
    out = torch.empty(8193, 4, device=DEV)
    assert _mean_seg(_x(14, rows=8193, ld=4), [(i, 1) for i in range(8193)], out=out)[0] == GSV_ERR_ARG      # more than 8192
