"""GPU: gsv_op_flash_attn64_seg, the segmented (variable-length) fused attention of the packed BERT pass, against torch fp32
softmax(Q K^T / 8) V per segment on the fp16-rounded inputs.  Bar: max-abs <= 4e-3, the one test_flash_attention_matches_sdpa
holds the row kernel to."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SEGS = {
    "one_row": [1],
    "edges": [16, 1, 17, 31, 32, 33, 3],       # off the 16-row tile, off the 32-key chunk, fewer chunks than waves
    "second_trip": [300, 5, 129],              # more than 8 chunks: the chunk loop takes a second trip
    "many": [26] * 40,
}


def _vt_halfs(lens, heads):
    return heads * 64 * 32 * sum((t + 31) // 32 for t in lens)


def _call(qkv, lens, heads, vt, out):
    from gsv import _lib
    seg = (C.c_int32 * max(len(lens), 1))(*lens)
    st = torch.cuda.current_stream()
    return _lib.lib().gsv_op_flash_attn64_seg(qkv.data_ptr(), len(lens), seg, heads, 0.125, vt.data_ptr(), out.data_ptr(),
                                              C.c_void_p(st.cuda_stream))


def _reference(qkv, lens, heads):
    inner = heads * 64
    x = qkv.float().cpu()
    outs, o = [], 0
    for t in lens:
        q, k, v = (x[o:o + t, i * inner:(i + 1) * inner].view(t, heads, 64).transpose(0, 1) for i in range(3))
        outs.append((torch.softmax(q @ k.transpose(1, 2) * 0.125, -1) @ v).transpose(0, 1).reshape(t, inner))
        o += t
    return torch.cat(outs)


@pytest.mark.parametrize("heads", [1, 3, 16])
@pytest.mark.parametrize("name", list(SEGS))
def test_segmented_attention_matches_per_segment_softmax(name, heads):
    from gsv import _lib
    from gsv import synthetic as S
    _lib.init(0)
    lens = SEGS[name]
    M, inner = sum(lens), heads * 64
    qkv = S.hash_symmetric(f"fa_seg_{name}", (M, 3 * inner), 1.5, 2).to(DEV, torch.float16)     # the row kernel test's inputs
    vt = torch.full((_vt_halfs(lens, heads),), float("nan"), dtype=torch.float16, device=DEV)    # a masked 0 x NaN would show
    out = torch.full((M, inner), float("nan"), dtype=torch.float16, device=DEV)
    _lib.check(_call(qkv, lens, heads, vt, out), "gsv_op_flash_attn64_seg")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(vt).all())
    err = (out.float().cpu() - _reference(qkv, lens, heads)).abs().max().item()
    print(f"[flash_seg] {name} heads {heads}: max-abs {err:.2e}")
    assert err <= 4e-3
    # isolation: other values in ONE segment's q / k / v leave every other segment's output bit-identical
    victim = len(lens) // 2
    o = sum(lens[:victim])
    qkv2 = qkv.clone()
    qkv2[o:o + lens[victim]] = S.hash_symmetric(f"fa_seg_other_{name}", (lens[victim], 3 * inner), 1.5, 3).to(DEV, torch.float16)
    out2 = torch.full_like(out, float("nan"))
    vt.fill_(float("nan"))
    _lib.check(_call(qkv2, lens, heads, vt, out2), "gsv_op_flash_attn64_seg")
    torch.cuda.synchronize()
    keep = torch.ones(M, dtype=torch.bool)
    keep[o:o + lens[victim]] = False
    assert torch.equal(out2.cpu()[keep], out.cpu()[keep])
    if len(lens) > 1:
        assert not torch.equal(out2.cpu()[~keep], out.cpu()[~keep])
    err2 = (out2.float().cpu() - _reference(qkv2, lens, heads)).abs().max().item()
    assert err2 <= 4e-3


def test_segmented_attention_refuses_bad_arguments():
    from gsv import _lib
    _lib.init(0)
    qkv = torch.zeros(8, 192, dtype=torch.float16, device=DEV)
    vt = torch.zeros(_vt_halfs([8], 1), dtype=torch.float16, device=DEV)
    out = torch.zeros(8, 64, dtype=torch.float16, device=DEV)
    assert _call(qkv, [], 1, vt, out) != 0                       # n_seg = 0
    assert b"segments" in _lib.lib().gsv_last_error()
    assert _call(qkv, [4, 0, 4], 1, vt, out) != 0                # a zero length
    assert b"length 0" in _lib.lib().gsv_last_error()
    assert _call(qkv, [8], 1, vt, out) == 0
    torch.cuda.synchronize()
