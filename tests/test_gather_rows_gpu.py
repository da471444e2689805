"""GPU: gsv_op_gather_rows, the row gather of the packed HuBERT pass: y[r] = x[idx[r]], a zero row for idx[r] < 0 and a NaN row for
idx[r] >= rows_in.  Bit-equal to torch.index_select with zero rows."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS_IN, ROWS_OUT = 97, 300


def _call(x, idx, y):
    from gsv import _lib
    _lib.init(0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return _lib.lib().gsv_op_gather_rows(x.data_ptr(), x.shape[0], idx.data_ptr(), idx.numel(), x.shape[1], y.data_ptr(),
                                         _lib.dtype_code(x.dtype), st)


def _indices():
    """valid rows in and out of order, repeats, the first and the last row, runs of -1 as between two audios"""
    g = torch.Generator().manual_seed(5)
    idx = torch.randint(0, ROWS_IN, (ROWS_OUT,), generator=g, dtype=torch.int32)
    idx[10:74] = -1
    idx[0], idx[1], idx[2], idx[3] = 0, ROWS_IN - 1, 0, ROWS_IN - 1
    idx[100:140] = torch.arange(20, 60, dtype=torch.int32)
    idx[200], idx[299] = -1, -7
    return idx


@pytest.mark.parametrize("dtype,ch", [(torch.float16, 768), (torch.float32, 512)])
def test_gather_is_bit_equal_to_index_select(dtype, ch):
    from gsv import _lib
    from gsv import synthetic as S
    x = S.hash_symmetric("gather_rows", (ROWS_IN, ch), 3.0, 1).to(DEV, dtype).contiguous()
    idx = _indices()
    y = torch.full((ROWS_OUT, ch), float("nan"), dtype=dtype, device=DEV)
    _lib.check(_call(x, idx.to(DEV), y), "gsv_op_gather_rows")
    torch.cuda.synchronize()
    ref = torch.index_select(x.cpu(), 0, idx.clamp(min=0).long())
    ref[idx < 0] = 0
    assert int((idx < 0).sum()) >= 66 and int((idx >= 0).sum()) > 200
    assert torch.equal(y.cpu().view(torch.uint8), ref.view(torch.uint8))
    # an index past the table gives a NaN row and leaves every other row as it was
    bad = idx.clone()
    bad[5], bad[150] = ROWS_IN, 2 ** 31 - 1
    y2 = torch.zeros_like(y)
    _lib.check(_call(x, bad.to(DEV), y2), "gsv_op_gather_rows")
    torch.cuda.synchronize()
    y2 = y2.cpu()
    assert bool(torch.isnan(y2[5]).all()) and bool(torch.isnan(y2[150]).all())
    keep = torch.ones(ROWS_OUT, dtype=torch.bool)
    keep[5] = keep[150] = False
    assert torch.equal(y2[keep].view(torch.uint8), ref[keep].view(torch.uint8))


def test_rows_that_are_no_multiple_of_16_bytes_are_refused():
    x = torch.zeros(4, 12, dtype=torch.float16, device=DEV)
    y = torch.zeros(2, 12, dtype=torch.float16, device=DEV)
    assert _call(x, torch.zeros(2, dtype=torch.int32, device=DEV), y) == -1
