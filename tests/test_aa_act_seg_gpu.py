"""GPU: the segmented form of BigVGAN's anti-aliased activation on channels-last rows (`gsv_op_aa_act_cl`, the kernel of
gsv_vocoder_forward_segments) against oracle/aa_oracle.py applied to each segment alone.

Layout: segments of 1, 2, 5, 6, 63, 64, 65 and 130 rows with gaps of 7 rows (385 rows, seven 64-row tiles): a 1-row segment
between two gaps inside a tile, segment edges on both sides of tile boundaries, a segment spanning three tiles.  C = 16 (part
of one 64-channel block) and 72 (one full block and a partial one).

Bars.  fp32: 1e-5 max-abs against the oracle, gap rows exactly 0.  fp16: the bar tests/test_vits_gpu.py sets for the plain
activation in fp16 against its golden (mean-abs <= 1e-3, max-abs <= 2e-2) -- the only fp16 bar the suite has for it."""
import ctypes as C
import functools

import pytest
import torch

from gsv import _lib
from oracle import aa_oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROWS = [1, 2, 5, 6, 63, 64, 65, 130]
GAP = 7


def _layout(rows=ROWS, gap=GAP):
    starts, t = [], 0
    for i, n in enumerate(rows):
        t += gap if i else 0
        starts.append(t)
        t += n
    seg = torch.full((t,), -1, dtype=torch.int32)
    for i, (a, n) in enumerate(zip(starts, rows)):
        seg[a:a + n] = i
    return starts, t, seg


@functools.lru_cache(maxsize=None)
def _case(Cn):
    """input rows [T][C] (gap rows 0), log-scale alpha / beta, and the oracle's output of every segment alone; computed once"""
    starts, T, seg = _layout()
    g = torch.Generator().manual_seed(100 + Cn)
    x = torch.randn(T, Cn, generator=g)
    x[seg < 0] = 0.0
    la, lb = torch.randn(Cn, generator=g) * 0.3, torch.randn(Cn, generator=g) * 0.3
    uf, df = aa_oracle.default_filters()
    ref = torch.zeros(T, Cn)
    for a, n in zip(starts, ROWS):
        ref[a:a + n] = aa_oracle.aa_activation(x[a:a + n].t().unsqueeze(0), la, lb, uf, df)[0].t()
    return x, la, lb, ref


def _act(x, la, lb, dtype, seg=None, starts=None, rows=None):
    """x [T][C] (cpu, fp32) through gsv_op_aa_act_cl in `dtype`; seg / starts / rows = the maps, or None for the plain kernel"""
    _lib.init(0)
    xd = x.to(DEV, dtype).contiguous()
    y = torch.full_like(xd, float("nan"))
    a, b = la.to(DEV, torch.float32).contiguous(), lb.to(DEV, torch.float32).contiguous()
    if seg is None:
        ptrs, n = (None, None, None), 0
        keep = ()
    else:
        keep = (seg.to(DEV), torch.tensor(starts, dtype=torch.int32, device=DEV), torch.tensor(rows, dtype=torch.int32, device=DEV))
        ptrs, n = tuple(t.data_ptr() for t in keep), len(rows)
    st = torch.cuda.current_stream(DEV)
    _lib.check(_lib.lib().gsv_op_aa_act_cl(xd.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1], a.data_ptr(), b.data_ptr(), 1,
                                           ptrs[0], ptrs[1], ptrs[2], n, _lib.dtype_code(dtype), C.c_void_p(st.cuda_stream)),
               "gsv_op_aa_act_cl")
    st.synchronize()
    del keep
    return y.float().cpu()


@pytest.mark.parametrize("Cn", [16, 72])
def test_fp32_each_segment_equals_the_oracle_alone(Cn):
    x, la, lb, ref = _case(Cn)
    starts, T, seg = _layout()
    y = _act(x, la, lb, torch.float32, seg, starts, ROWS)
    assert torch.isfinite(y).all(), "every row and channel is written"
    assert torch.equal(y[seg < 0], torch.zeros_like(y[seg < 0])), "gap rows are stored as 0"
    for a, n in zip(starts, ROWS):
        err = (y[a:a + n] - ref[a:a + n]).abs().max().item()
        print(f"C={Cn} segment of {n} rows at {a}: max |engine - oracle| = {err:.3e}")
        assert err <= 1e-5


@pytest.mark.parametrize("Cn", [16, 72])
def test_fp16_within_the_plain_activations_bar(Cn):
    x, la, lb, ref = _case(Cn)
    starts, T, seg = _layout()
    y = _act(x, la, lb, torch.float16, seg, starts, ROWS)
    assert torch.equal(y[seg < 0], torch.zeros_like(y[seg < 0]))
    err = y - ref
    live = err[seg >= 0]
    print(f"C={Cn} fp16: mean-abs {live.abs().mean().item():.3e}, max-abs {live.abs().max().item():.3e}")
    assert live.abs().mean().item() <= 1e-3 and live.abs().max().item() <= 2e-2


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_no_leakage_from_gaps_or_neighbours(dtype):
    """gap rows of the input at 1e4 and every other segment scaled: the untouched segments come out bit-equal"""
    x, la, lb, _ = _case(72)
    starts, T, seg = _layout()
    base = _act(x, la, lb, dtype, seg, starts, ROWS)
    for parity in (0, 1):
        z = x.clone()
        z[seg < 0] = 1e4
        for i, (a, n) in enumerate(zip(starts, ROWS)):
            if i % 2 == parity:
                z[a:a + n] *= 3.0 + i
        y = _act(z, la, lb, dtype, seg, starts, ROWS)
        assert torch.equal(y[seg < 0], torch.zeros_like(y[seg < 0]))
        for i, (a, n) in enumerate(zip(starts, ROWS)):
            if i % 2 != parity:
                assert torch.equal(y[a:a + n], base[a:a + n]), f"segment {i} changed with its neighbours and the gaps"
            else:
                assert not torch.equal(y[a:a + n], base[a:a + n])


@pytest.mark.parametrize("T,Cn", [(1, 16), (130, 72), (200, 16)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_one_segment_with_a_map_equals_the_plain_kernel(T, Cn, dtype):
    g = torch.Generator().manual_seed(T)
    x = torch.randn(T, Cn, generator=g)
    la, lb = torch.randn(Cn, generator=g) * 0.3, torch.randn(Cn, generator=g) * 0.3
    plain = _act(x, la, lb, dtype)
    mapped = _act(x, la, lb, dtype, torch.zeros(T, dtype=torch.int32), [0], [T])
    assert torch.equal(plain, mapped)
    if dtype == torch.float32:
        uf, df = aa_oracle.default_filters()
        ref = aa_oracle.aa_activation(x.t().unsqueeze(0), la, lb, uf, df)[0].t()
        assert (plain - ref).abs().max().item() <= 1e-5


def test_a_map_without_its_tables_is_an_error():
    _lib.init(0)
    x = torch.zeros(8, 16, device=DEV)
    ab = torch.zeros(16, device=DEV)
    seg = torch.zeros(8, dtype=torch.int32, device=DEV)
    rc = _lib.lib().gsv_op_aa_act_cl(x.data_ptr(), x.data_ptr(), 8, 16, ab.data_ptr(), ab.data_ptr(), 1, seg.data_ptr(), None, None, 1,
                                     _lib.GSV_F32, None)
    assert rc != 0
