"""GPU: gsv_op_lora_delta (csrc/lora.hip), the per-row low-rank delta of the adapted DiT passes, against an fp64 mirror with a
per-element bar built like tests/_convref.py's.

What the kernel does, and what the mirror therefore does: x, the factors and y are stored in the engine dtype; u = x A^T
accumulates in fp32 over K and, in fp16, is rounded to fp16 once (it is parked in LDS as the second product's operand); the
rank contraction accumulates in fp32; y_new = y + gate * (u B^T) is rounded to the output dtype once.

Bar per output element:  ulp_out(|ref|) + |gate| sum_q delta_u[q] |B[c][q]| + 16 sqrt(r) 2^-24 (|y| + |gate| sum_q |u_q B[c][q]|)
  delta_u = 16 sqrt(K) 2^-24 sum_k |x_k A[q][k]|  (+ in fp16 one fp16 ulp of |u| + that: the rounding of u), the error of the
  first product carried through the second; the last term is the fp32 accumulation of the rank contraction and the epilogue."""
import ctypes as C
import math

import pytest
import torch

from _convref import U32, check, ulp
from gsv import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SLOTS = [1, -1, 0, 1, 2]
GUARD = 4096


def _case(K, N, n_proj, ranks, dtype, tag):
    """the store: per slot the stacked factors A [n_proj][r][K], B [N][r] in the engine dtype (cpu), and their packed blocks
    (A [n_proj * rp][K] then B [N][rp], rank padded with zeros)"""
    store = []
    for s, r in enumerate(ranks):
        rp = (r + 15) // 16 * 16
        a = S.hash_symmetric(f"{tag}_A{s}", (n_proj, r, K), 2.0 / math.sqrt(K), 40 + s).to(dtype)
        b = S.hash_symmetric(f"{tag}_B{s}", (N, r), 1.0 / math.sqrt(r), 50 + s).to(dtype)
        ap = torch.zeros(n_proj, rp, K, dtype=dtype)
        ap[:, :r] = a
        bp = torch.zeros(N, rp, dtype=dtype)
        bp[:, :r] = b
        store.append(dict(r=r, rp=rp, a=a, b=b, block=torch.cat([ap.reshape(-1), bp.reshape(-1)])))
    return store


def _mirror(x, y0, gate, store, slots, Tn, n_proj, dtype):
    """fp64 reference and bar, [DB * Tn][N]"""
    K, N = x.shape[1], y0.shape[1]
    npc = N // n_proj
    ref = y0.to(torch.float64).clone()
    bar = torch.zeros_like(ref)       # stays 0 on rows without a slot: those must be bit-unchanged
    g = torch.ones(N, dtype=torch.float64) if gate is None else gate.to(torch.float64)
    for b, s in enumerate(slots):
        if s < 0:
            continue
        rows = slice(b * Tn, (b + 1) * Tn)
        xb = x[rows].to(torch.float64)
        yb = y0[rows].to(torch.float64)
        st = store[s]
        d = torch.zeros(Tn, N, dtype=torch.float64)
        mag = torch.zeros_like(d)
        prop = torch.zeros_like(d)
        for p in range(n_proj):
            A = st["a"][p].to(torch.float64)                   # [r][K]
            Bm = st["b"][p * npc:(p + 1) * npc].to(torch.float64)     # [npc][r]
            u = xb @ A.t()
            delta = 16 * math.sqrt(K) * U32 * (xb.abs() @ A.abs().t())
            if dtype == torch.float16:
                delta = delta + ulp(u.abs() + delta, torch.float16)
                u = u.to(torch.float32).half().to(torch.float64)
            d[:, p * npc:(p + 1) * npc] = u @ Bm.t()
            mag[:, p * npc:(p + 1) * npc] = u.abs() @ Bm.abs().t()
            prop[:, p * npc:(p + 1) * npc] = delta @ Bm.abs().t()
        ref[rows] = yb + g * d
        bar[rows] = ulp(ref[rows], dtype) + g.abs() * prop + 16 * math.sqrt(st["r"]) * U32 * (yb.abs() + g.abs() * mag)
    return ref, bar


@pytest.mark.parametrize("ranks", [(4, 16, 40, 128), (128, 40, 16, 4)], ids=["r4-16-40-128", "r128-40-16-4"])
@pytest.mark.parametrize("Tn", [1, 37, 64, 70])
@pytest.mark.parametrize("K,N,n_proj,gated", [(128, 384, 3, False), (128, 128, 1, True)], ids=["qkv", "out"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_delta_against_the_fp64_mirror(dtype, K, N, n_proj, gated, Tn, ranks):
    from gsv import _lib
    _lib.init(0)
    DB = len(SLOTS)
    tag = f"ld{K}_{N}_{Tn}"
    store = _case(K, N, n_proj, ranks, dtype, tag)
    x = S.hash_symmetric(tag + "_x", (DB * Tn, K), 1.0, 1).to(dtype)
    y0 = S.hash_symmetric(tag + "_y", (DB * Tn, N), 1.0, 2).to(dtype)
    gate = S.hash_symmetric(tag + "_g", (N,), 1.5, 3) if gated else None
    with torch.cuda.device(DEV):
        xd = x.to(DEV).contiguous()
        n = DB * Tn * N
        yd = torch.full((n + GUARD,), float("nan"), device=DEV, dtype=dtype)
        yd[:n] = y0.to(DEV).reshape(-1)
        gd = gate.to(DEV).contiguous() if gated else None
        blocks = [st["block"].to(DEV).contiguous() for st in store]
        torch.cuda.synchronize()
        rc = _lib.lib().gsv_op_lora_delta(xd.data_ptr(), yd.data_ptr(), Tn, DB, K, N, n_proj, (C.c_int * DB)(*SLOTS), len(store),
                                          (C.c_void_p * len(store))(*[b.data_ptr() for b in blocks]),
                                          (C.c_int * len(store))(*[st["rp"] for st in store]), gd.data_ptr() if gated else None,
                                          _lib.dtype_code(dtype), None)
        _lib.check(rc, "gsv_op_lora_delta")
        torch.cuda.synchronize()
        got = yd.cpu()
    assert torch.isnan(got[n:]).all(), "the NaN sentinels behind y"
    got = got[:n].reshape(DB * Tn, N)
    for b, s in enumerate(SLOTS):
        if s < 0:
            assert torch.equal(got[b * Tn:(b + 1) * Tn], y0[b * Tn:(b + 1) * Tn]), "a row without a slot is not touched"
    ref, bar = _mirror(x, y0, gate, store, SLOTS, Tn, n_proj, dtype)
    moved = (ref - y0.to(torch.float64)).abs().max().item()
    live = torch.tensor([s >= 0 for s in SLOTS]).repeat_interleave(Tn)      # the other rows were compared bit for bit above
    worst = check(got[live], ref[live], bar[live], f"lora_delta {tag}")
    print(f"[lora_delta] {tag} {dtype} ranks {ranks}: worst err / bar {worst:.3f}, largest delta {moved:.3f}")
    assert moved > 0.1, "the case must move y by far more than the bar"


def test_bad_arguments_are_refused():
    from gsv import _lib
    _lib.init(0)
    with torch.cuda.device(DEV):
        x = torch.zeros(64, 128, device=DEV, dtype=torch.float16)
        y = torch.full((64 * 128,), float("nan"), device=DEV, dtype=torch.float16)
        blk = torch.zeros(16 * 128 + 128 * 16, device=DEV, dtype=torch.float16)

        def call(K=128, N=128, n_proj=1, slots=(0,), rp=16, Tn=64):
            return _lib.lib().gsv_op_lora_delta(x.data_ptr(), y.data_ptr(), Tn, len(slots), K, N, n_proj, (C.c_int * len(slots))(*slots),
                                                1, (C.c_void_p * 1)(blk.data_ptr()), (C.c_int * 1)(rp), None, _lib.GSV_F16, None)
        assert call(slots=(1,)) != 0          # slot outside the store
        assert call(slots=(-2,)) != 0
        assert call(rp=8) != 0                # not padded to 16
        assert call(rp=144) != 0              # beyond rank 128
        assert call(K=100) != 0               # K not a multiple of 32
        assert call(N=120) != 0               # N not a multiple of 16
        assert call(n_proj=4) != 0
        torch.cuda.synchronize()
        assert torch.isnan(y).all()
