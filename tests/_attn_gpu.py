"""What the GPU tests of the fused and materialised attention kernels share: one call of each hook on NaN-filled outputs with
guard rows, read back to the host.  Mirror, bars and inputs are tests/_attnmirror.py's."""
import ctypes as C

import torch

import _attnmirror as M

DEV = "cuda:0"
GUARD = 64          # NaN rows behind every `out`
PAD = 8             # rows between two utterances of the rows hook (include/gsv.h)
NAN = float("nan")
FAMILY = {1: "rows", 2: "seg", 3: "rel96", 4: "materialised"}


def lib():
    from gsv import _lib
    _lib.init(0)
    return _lib.lib()


def ints(v):
    return (C.c_int32 * max(len(v), 1))(*v)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def last_route():
    """(family name, QT) of the last attention launch; the record is cleared"""
    r = int(lib().gsv_debug_last_attn_route(1))
    return FAMILY.get(r & 255, r & 255), (r >> 8) & 255


def rows_call(qkvs, H, qt, cs=None, rope_half=0, scale=0.125):
    """gsv_op_flash_attn64_rows on the utterances qkvs (each [T][3 H 64] fp16, host) laid out with the hook's padded strides;
    everything the kernel may not read or write is NaN.  -> rc, out [rows][T + 8][H 64] (host), guard rows, the qkv buffer read
    back (the rotary runs in place) [rows][T + 8][3 H 64], the V^T scratch [rows][H 64 ceil32(T) + 64]"""
    l = lib()
    rows, T, inner = len(qkvs), qkvs[0].shape[0], H * 64
    ldv = (T + 31) // 32 * 32
    buf = torch.full((rows, T + PAD, 3 * inner), NAN, dtype=torch.float16)
    for r, x in enumerate(qkvs):
        buf[r, :T] = x
    buf_d = buf.to(DEV)
    out = torch.full((rows * (T + PAD) + GUARD, inner), NAN, dtype=torch.float16, device=DEV)
    vt = torch.full((rows, inner * ldv + 64), NAN, dtype=torch.float16, device=DEV)
    cs_d = cs.to(DEV).contiguous() if cs is not None else None
    torch.cuda.synchronize()
    l.gsv_debug_last_attn_route(1)
    rc = l.gsv_op_flash_attn64_rows(buf_d.data_ptr(), T, H, rows, scale, cs_d.data_ptr() if cs is not None else None, rope_half, qt,
                                    vt.data_ptr(), out.data_ptr(), None)
    torch.cuda.synchronize()
    o = out.cpu()
    return rc, o[:rows * (T + PAD)].reshape(rows, T + PAD, inner), o[rows * (T + PAD):], buf_d.cpu(), vt.cpu()


def seg_call(qkv, lens, H, qt, scale=0.125):
    """gsv_op_flash_attn64_seg_qt (qt None: the existing gsv_op_flash_attn64_seg) -> rc, out [sum T][H 64], guard rows, V^T"""
    l = lib()
    Mr, inner = sum(lens), H * 64
    qkv_d = qkv.to(DEV)
    out = torch.full((Mr + GUARD, inner), NAN, dtype=torch.float16, device=DEV)
    vt = torch.full((inner * 32 * sum((t + 31) // 32 for t in lens),), NAN, dtype=torch.float16, device=DEV)
    torch.cuda.synchronize()
    l.gsv_debug_last_attn_route(1)
    if qt is None:
        rc = l.gsv_op_flash_attn64_seg(qkv_d.data_ptr(), len(lens), ints(lens), H, scale, vt.data_ptr(), out.data_ptr(), None)
    else:
        rc = l.gsv_op_flash_attn64_seg_qt(qkv_d.data_ptr(), len(lens), ints(lens), H, scale, qt, vt.data_ptr(), out.data_ptr(), None)
    torch.cuda.synchronize()
    o = out.cpu()
    return rc, o[:Mr], o[Mr:], vt.cpu()


def attn_call(q2, kv2, H, kc, route, rel=(None, None), kr=None, packed=False, scale=None):
    """gsv_op_attention.  packed: q2 is the self form's [T][3 H kc] (q == kv, as the encoders call it), else q2 [Tq][H kc] and
    kv2 [Tk][2 H kc].  -> rc, out [Tq][H kc] (host), guard rows"""
    from gsv import _lib
    l = lib()
    dt = q2.dtype
    hk = H * kc
    q_d = q2.to(DEV)
    kv_d = q_d if packed else kv2.to(DEV)
    Tq, Tk = q2.shape[0], (q2.shape[0] if packed else kv2.shape[0])
    rk, rv = (t.to(DEV) if t is not None else None for t in rel)
    out = torch.full((Tq + GUARD, hk), NAN, dtype=dt, device=DEV)
    krh = ints(kr.flatten().tolist()) if kr is not None else None
    torch.cuda.synchronize()
    l.gsv_debug_last_attn_route(1)
    rc = l.gsv_op_attention(q_d.data_ptr(), 3 * hk if packed else hk, 0, kv_d.data_ptr(), 3 * hk if packed else 2 * hk,
                            hk if packed else 0, 2 * hk if packed else hk, Tq, Tk, H, kc, scale if scale is not None else kc ** -0.5,
                            rk.data_ptr() if rk is not None else None, rv.data_ptr() if rv is not None else None, krh,
                            _lib.dtype_code(dt), route, out.data_ptr(), hk, None)
    torch.cuda.synchronize()
    o = out.cpu()
    return rc, o[:Tq], o[Tq:]


class Worst:
    """worst err / bar per (route, regime), for the summary test of each file"""

    def __init__(self, tag):
        self.tag, self.w = tag, {}

    def add(self, route, regime, worst, what):
        self.w[(route, regime)] = max(self.w.get((route, regime), 0.0), worst)
        print(f"[{self.tag}] {what}: worst err/bar {worst:.3f}")

    def report(self):
        for (route, regime), v in sorted(self.w.items()):
            print(f"[{self.tag}] worst err/bar, {route}, {regime}: {v:.3f}")
        assert self.w and all(v <= 1.0 for v in self.w.values())
