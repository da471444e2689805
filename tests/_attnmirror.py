"""The fused (csrc/attn.hip) and materialised (csrc/engine.hip) attention kernels restated for the tests, beside _attnref.py
(the AR prefill's): one float64 mirror for every form, the per-element bars, the inputs of the three regimes, the shape tables,
CPU emulations of each route's arithmetic (what the bars are sized against) and the refusal table of the hooks.

Layout, as the hooks take it: qkv [T][3 * H * D] = [q | k | v] column blocks, head h at columns h * D ..; out [T][H * D].
Forms: plain softmax attention (D = 64: flash_attn64 rows / segments; any D materialised), the window-4 relative-position form of
enc_p (attentions.py:227-258: a key bias (q_i / sqrt(D)) . rel_k[j - i + 4] on |j - i| <= 4 and a value term
sum_r p[i][i + r - 4] rel_v[r]), per-query key ranges kr[i] = [lo, hi) (the segmented decode), and Tq != Tk (MRTE).
"""
import math

import torch

W, NB = 4, 9                 # relative window, band width 2 W + 1
CHUNK, WAVES = 32, 4         # keys per chunk, chunk c -> wave (c - c0) % 4
REGIMES = ("flat", "sharp", "adversarial")
QK_SCALE = {"flat": 0.5, "sharp": 2.0, "adversarial": 2.0}
RELK_AMP = {"flat": 0.3, "sharp": 1.5, "adversarial": 1.5}
NINF = -float("inf")

# ---- shape tables ---------------------------------------------------------------------------------------------------------
# rows kernel: T on every side of its edges (16-row sub-tile, 32-key chunk, 64-row QT 4 tile, 4 waves, trips of 8 chunks)
ROWS_T = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 128, 129, 256, 257, 385, 640]
ROWS_HEADS = [(33, 1), (129, 3), (65, 5)]                     # workgroup counts of several residues mod 8 (the XCD remap)
ROWS_AUTO = [((40, 100), 2), ((70, 100), 4), ((33, 2), 1)]    # (T, heads) -> QT the launcher's rule must record
ROPE_CASES = [(1, 2, 32, 1), (33, 2, 32, 1), (257, 2, 32, 1), (33, 16, 32, 1), (33, 2, 12, 1), (33, 2, 32, 3), (257, 2, 12, 3)]  # T, heads, rope_half, rows
SEGS = {   # the first four are tests/test_flash_attn_seg_gpu.py's
    "one_row": [1],
    "edges": [16, 1, 17, 31, 32, 33, 3],
    "second_trip": [300, 5, 129],
    "many": [26] * 40,
    "on_boundaries": [16, 32, 64, 15, 33, 63, 65, 128],      # segments that end on a 16 / 32 / 64 boundary and beside one
}
REL_T = [1, 4, 5, 9, 31, 32, 33, 36, 129, 257, 300]
# key-range layouts (segments [lo, hi) on one time axis, gap rows between them), T
RANGE_LAYOUTS = {
    "three": ([(0, 37), (40, 70), (77, 150)], 150),           # second segment starts off a 32 boundary; tile 32..63 spans two
    "gap_first": ([(3, 30), (35, 60), (64, 100)], 104),       # tile 0 and tile 2 start on a gap row and end inside a segment
    "short": ([(0, 1), (3, 5), (8, 40), (43, 44), (47, 49)], 52),   # segments of 1 and 2 rows: shorter than the band
    "six": ([(0, 90), (93, 200), (203, 290), (296, 420), (423, 500), (505, 600)], 603),
}
MAT_SELF_T = [1, 7, 8, 9, 33, 129, 300]                       # Tk = 7, 8, 9: both sides of P's padding to 8 (fp16) / 4 (fp32)
CROSS = [(50, 7), (7, 50), (130, 33)]                         # (Tq, Tk), kc 128, heads 4
LONG = (3, 12300)                                             # the branch of softmax_rows_kernel that does not cache the row


def seed_of(*key):
    s = 17
    for x in key:
        x = REGIMES.index(x) if isinstance(x, str) else int(x)
        s = (s * 1315423911 + 2654435761 * (x + 3) + 40503) % (2 ** 61 - 1)
    return s


def split(qkv, H, D):
    """[T][3 H D] -> q, k, v [H][T][D]"""
    T = qkv.shape[0]
    return tuple(qkv[:, c * H * D:(c + 1) * H * D].reshape(T, H, D).transpose(0, 1) for c in range(3))


def merge(o):
    """[H][T][D] -> [T][H D]"""
    return o.transpose(0, 1).reshape(o.shape[1], -1)


def self_ranges(segs, T):
    """kr [T][2] as vits.hip builds it for self-attention: a segment's rows see the segment, a gap row t sees [t, t + 1)"""
    kr = torch.stack([torch.arange(T), torch.arange(T) + 1], dim=1)
    for lo, hi in segs:
        kr[lo:hi, 0], kr[lo:hi, 1] = lo, hi
    return kr.int()


def cross_ranges(qsegs, ksegs, Tq):
    """kr [Tq][2] of the cross form: query segment s sees key segment s, gap rows see [0, 0)"""
    kr = torch.zeros(Tq, 2, dtype=torch.int32)
    for (ql, qh), (kl, kh) in zip(qsegs, ksegs):
        kr[ql:qh, 0], kr[ql:qh, 1] = kl, kh
    return kr


def visible(kr, Tq, Tk):
    if kr is None:
        return torch.ones(Tq, Tk, dtype=torch.bool)
    j = torch.arange(Tk)[None, :]
    return (j >= kr[:, 0:1]) & (j < kr[:, 1:2])


def _band_index(Tq, Tk):
    r = torch.arange(Tk)[None, :] - torch.arange(Tq)[:, None] + W
    return r, (r >= 0) & (r < NB)


def attn_ref(q, k, v, scale, rel_k=None, rel_v=None, kr=None, parts=False):
    """float64 mirror on the values given (already rounded to the kernel's dtype): q [H][Tq][D], k / v [H][Tk][D] ->
    ref [Tq][H D] and A = P |v| + band |rel_v| (what the probabilities multiply: the scale of the fp16-P error).  Rows with an
    empty range give 0 in both.  parts: also the P v term alone (the materialised path rounds it before the relative term)."""
    q, k, v = q.double(), k.double(), v.double()
    H, Tq, _ = q.shape
    Tk = k.shape[1]
    s = q @ k.transpose(1, 2) * scale
    vis = visible(kr, Tq, Tk)
    if rel_k is not None:
        r, band = _band_index(Tq, Tk)
        b = (q @ rel_k.double().t()) * scale                       # [H][Tq][9]
        s = s + torch.where(band, b.gather(2, r.clamp(0, NB - 1).expand(H, Tq, Tk)), torch.zeros((), dtype=torch.float64))
    empty = ~vis.any(dim=1)
    s = s.masked_fill(~vis, NINF)
    s[:, empty] = 0.0
    p = torch.softmax(s, dim=-1)
    p[:, empty] = 0.0
    pv, A = p @ v, p @ v.abs()
    ref = pv.clone()
    if rel_v is not None:
        pb = torch.zeros(H, Tq, NB, dtype=torch.float64)
        i = torch.arange(Tq)
        for rr in range(NB):
            j = i + rr - W
            ok = (j >= 0) & (j < Tk)
            pb[:, i[ok], rr] = p[:, i[ok], j[ok]]                   # 0 where the key is outside the range: p is 0 there
        ref = ref + pb @ rel_v.double()
        A = A + pb @ rel_v.double().abs()
    if parts:
        return merge(ref), merge(A), merge(pv)
    return merge(ref), merge(A)


def seg_attn_ref(qkv, lens, H, D, scale):
    """packed segments, each attending to itself (flash_attn64_seg): ref, A [sum T][H D] and the per-row segment length"""
    refs, As, n, o = [], [], [], 0
    for t in lens:
        r, a = attn_ref(*split(qkv[o:o + t], H, D), scale)
        refs.append(r); As.append(a); n.append(torch.full((t, 1), float(t), dtype=torch.float64))
        o += t
    return torch.cat(refs), torch.cat(As), torch.cat(n)


# ---- bars ------------------------------------------------------------------------------------------------------------------

def flash_bar(ref, A, n):
    """the project's flash bar (DESIGN.md "Mirror and bars"): fp16 output rounding + probabilities rounded to fp16 before the PV
    MFMA + n keys whose probability may be an fp16 subnormal; n = the sequence's own length (a number, or one per row)"""
    return 2.0 ** -11 * ref.abs() + 2.0 ** -11 * A + n * 2.0 ** -25


def mat_f16_bar(ref, A, pv, Tk, rel):
    """materialised fp16: P = fp16(p) feeds the PV GEMM (2^-11 A, and Tk 2^-25 for subnormal p, as in the flash bar), the GEMM
    stores fp16 (2^-11 |P v|), and with a relative term relv_add_kernel re-reads that fp16, adds the band term in fp32 and
    rounds again (2^-11 |ref|).  Without the term P v IS ref: one output rounding."""
    bar = 2.0 ** -11 * A + Tk * 2.0 ** -25 + 2.0 ** -11 * ref.abs()
    return bar + 2.0 ** -11 * pv.abs() if rel else bar


def mat_f32_bar(ref):
    """the project's fp32 attention tolerance for |v| <= 1 (decode and prefill scalar kernels)"""
    return torch.full_like(ref, 2e-5)


def rope_bar(ref, a, b):
    """one fp16 rounding of the result + three fp32 roundings (two products and their difference / sum) of terms <= |a| + |b|"""
    return 2.0 ** -11 * ref.abs() + 2.0 ** -25 + 2.0 ** -22 * (a.abs() + b.abs())


def check(out, ref, bar, what=""):
    """worst err / bar; AssertionError if an element lies outside its bar (or is not finite)"""
    o = out.double()
    assert torch.isfinite(o).all(), f"{what}: non-finite output"
    err = (o - ref).abs()
    ratio = torch.where(bar > 0, err / bar, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    worst = float(ratio.max())
    if worst > 1.0:
        i = int(ratio.argmax())
        r, c = i // ref.shape[1], i % ref.shape[1]
        raise AssertionError(f"{what}: element [{r}, {c}] outside the bar: got {float(o[r, c])!r}, mirror {float(ref[r, c])!r}, "
                             f"bar {float(bar[r, c]):.3e}, err/bar {worst:.3f}; {int((ratio > 1).sum())} elements outside")
    return worst


# ---- inputs ----------------------------------------------------------------------------------------------------------------

def make_qkv(T, H, D, regime, dtype, seed=0, segs=None, Tk=None, ksegs=None):
    """q, k randn * QK_SCALE, v uniform in [-1, 1].  Self form (Tk None): one [T][3 H D] matrix.  Cross form: (q [T][H D],
    kv [Tk][2 H D]).  adversarial with segments: the queries of a segment share a component, and the keys just outside the
    segment's range (hi and lo - 1; in the cross form of the segment's KEY range) are 1.5 x the segment's mean query, so
    a range off by one at either end hands most of every row's mass to a hidden key."""
    g = torch.Generator().manual_seed(seed_of(T, H, D, regime, seed, Tk or 0, *(x for s_ in (segs or []) for x in s_)))
    sc = QK_SCALE[regime]
    Tkk = T if Tk is None else Tk
    q = torch.randn(T, H, D, generator=g) * sc
    k = torch.randn(Tkk, H, D, generator=g) * sc
    v = torch.rand(Tkk, H, D, generator=g) * 2 - 1
    if regime == "adversarial" and segs:
        for n, (lo, hi) in enumerate(segs):
            q[lo:hi] += torch.randn(1, H, D, generator=g) * sc
            mean = q[lo:hi].mean(0)
            kl, kh = (lo, hi) if ksegs is None else ksegs[n]
            for j in (kh, kl - 1):
                if 0 <= j < Tkk:
                    k[j] = 1.5 * mean if not _is_claimed(j, segs if ksegs is None else ksegs, n) else k[j] + 1.5 * mean
    if Tk is None:
        return torch.cat([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], dim=1).to(dtype)
    return q.reshape(T, -1).to(dtype), torch.cat([k.reshape(Tkk, -1), v.reshape(Tkk, -1)], dim=1).to(dtype)


def _is_claimed(j, segs, n):
    """row j is already the boundary key of an earlier segment (a gap of one row): it then carries both pulls"""
    return any(j in (hi, lo - 1) for lo, hi in segs[:n])


def make_rel(D, regime, seed=0, qkv=None, segs=None, H=None):
    """rel_k, rel_v fp32 [9][D].  adversarial: the rel_k rows of every offset but 0 point along the mean query of all
    segments, so the bias of a band key is large wherever the band leaves a segment: added to a hidden key it would win."""
    g = torch.Generator().manual_seed(seed_of(D, regime, seed, 77))
    rel_k = torch.randn(NB, D, generator=g) * RELK_AMP[regime]
    rel_v = torch.rand(NB, D, generator=g) * 2 - 1
    if regime == "adversarial" and qkv is not None and segs:
        q = split(qkv.float(), H, D)[0]                            # [H][T][D]
        rows = torch.cat([torch.arange(lo, hi) for lo, hi in segs])
        u = q[:, rows].mean(dim=(0, 1))
        u = u / u.norm()
        for rr in range(NB):
            if rr != W:
                rel_k[rr] = 6.0 * u
    return rel_k.contiguous(), rel_v.contiguous()


def hidden_mass_fraction(q, k, scale, kr, rel_k=None):
    """of the (query, head) pairs with a hidden key: the fraction whose UNMASKED softmax (band bias on every band key) puts
    >= 0.5 of its mass on keys outside the query's range"""
    q, k = q.double(), k.double()
    H, Tq, _ = q.shape
    Tk = k.shape[1]
    s = q @ k.transpose(1, 2) * scale
    if rel_k is not None:
        r, band = _band_index(Tq, Tk)
        b = (q @ rel_k.double().t()) * scale
        s = s + torch.where(band, b.gather(2, r.clamp(0, NB - 1).expand(H, Tq, Tk)), torch.zeros((), dtype=torch.float64))
    p = torch.softmax(s, dim=-1)
    vis = visible(kr, Tq, Tk)
    has = ~vis.all(dim=1)
    hidden = (p * (~vis)).sum(-1)[:, has]
    return float((hidden >= 0.5).sum()) / hidden.numel() if hidden.numel() else 1.0


def heads_of(x, H, D):
    """[T][H D] -> [H][T][D]"""
    return x.reshape(x.shape[0], H, D).transpose(0, 1)


def cross_layout(Tq, Tk):
    """the cross form's ranges: two query segments with a gap row between and behind them, each seeing its own half of the keys"""
    a, b = max(Tq // 2 - 1, 1), Tq - 1
    qsegs = [(0, a), (a + 1, b)] if b > a + 1 else [(0, a)]
    h = Tk // 2
    return qsegs, [(0, h), (h, Tk)][:len(qsegs)]


_CACHE = {}


def cross_case(Tq, Tk, regime, dtype, H=4, D=128):
    """MRTE's shape: (q2 [Tq][H D], kv2 [Tk][2 H D]) as the hook takes them, their heads, kr, and the mirror's (ref, A, pv)"""
    key = ("cross", Tq, Tk, regime, dtype, H, D)
    if key not in _CACHE:
        qsegs, ksegs = cross_layout(Tq, Tk)
        q2, kv2 = make_qkv(Tq, H, D, regime, dtype, segs=qsegs, Tk=Tk, ksegs=ksegs)
        kr = cross_ranges(qsegs, ksegs, Tq)
        q, k, v = heads_of(q2, H, D), heads_of(kv2[:, :H * D], H, D), heads_of(kv2[:, H * D:], H, D)
        _CACHE[key] = ((q2, kv2), q, (k, v), kr, attn_ref(q, k, v, 1 / math.sqrt(D), kr=kr, parts=True))
    return _CACHE[key][1:]


def cross_case_packed(Tq, Tk, regime, dtype, H=4, D=128):
    cross_case(Tq, Tk, regime, dtype, H, D)
    return _CACHE[("cross", Tq, Tk, regime, dtype, H, D)][0]


def long_case(dtype, packed=False):
    """Tq = 3 queries over Tk = 12300 keys with the band (keys i - 4 .. i + 4 of query i) and ranges, one head of 96"""
    key = ("long", dtype)
    if key not in _CACHE:
        Tq, Tk = LONG
        q2, kv2 = make_qkv(Tq, 1, 96, "sharp", dtype, Tk=Tk)
        rel = make_rel(96, "sharp")
        kr = torch.tensor([[0, Tk], [1, 12290], [2, Tk]], dtype=torch.int32)
        q, k, v = heads_of(q2, 1, 96), heads_of(kv2[:, :96], 1, 96), heads_of(kv2[:, 96:], 1, 96)
        _CACHE[key] = ((q2, kv2), q, (k, v), rel, kr, attn_ref(q, k, v, 1 / math.sqrt(96), rel[0], rel[1], kr, parts=True))
    return _CACHE[key][0] if packed else _CACHE[key][1:]


# ---- rotary ----------------------------------------------------------------------------------------------------------------

def rope_table(T, rope_half, dim_head=64):
    """cos | sin [T][rope_half][2] fp32 of x_transformers' RotaryEmbedding(dim_head) (oracle/rope.py): pair p turns by
    t * base^(-2p / dim_head)"""
    inv = 1.0 / (10000 ** (torch.arange(0, dim_head, 2).float() / dim_head))
    f = torch.arange(T).float()[:, None] * inv[None, :rope_half]
    return torch.stack([f.cos(), f.sin()], dim=-1).contiguous()


def rope_ref(qkv, cs, rope_half, H, D=64, pairing="interleaved", every_head=False):
    """float64 rotation of the q and k blocks of qkv [T][3 H D] on the first 2 * rope_half channels of the UN-SPLIT projection
    (so head 0 only at rope_half = 32), pairs (2p, 2p + 1) -> ref [T][3 H D] and its bar (0 on the channels that must stay
    bit-unchanged: the rest of q and k, all of v).  pairing / every_head: the two mutants."""
    x = qkv.double()
    ref, bar = x.clone(), torch.zeros_like(x)
    c, s = cs[..., 0].double(), cs[..., 1].double()
    n = 2 * rope_half
    starts = [blk * H * D + (h * D if every_head else 0) for blk in (0, 1) for h in (range(H) if every_head else (0,))]
    for o in starts:
        if pairing == "interleaved":
            ia, ib = torch.arange(0, n, 2) + o, torch.arange(1, n, 2) + o
        else:
            ia, ib = torch.arange(rope_half) + o, torch.arange(rope_half) + rope_half + o
        a, b = x[:, ia], x[:, ib]
        ref[:, ia], ref[:, ib] = a * c - b * s, b * c + a * s
        bar[:, ia] = rope_bar(ref[:, ia], a, b)
        bar[:, ib] = rope_bar(ref[:, ib], a, b)
    return ref, bar


def rope_emulate(qkv, cs, rope_half, H, D=64, pairing="interleaved", every_head=False):
    """vt_kernel's rotary plane on fp16 qkv: fp32 products and sum, one fp16 rounding"""
    out = qkv.clone()
    x = qkv.float()
    c, s = cs[..., 0], cs[..., 1]
    n = 2 * rope_half
    starts = [blk * H * D + (h * D if every_head else 0) for blk in (0, 1) for h in (range(H) if every_head else (0,))]
    for o in starts:
        if pairing == "interleaved":
            ia, ib = torch.arange(0, n, 2) + o, torch.arange(1, n, 2) + o
        else:
            ia, ib = torch.arange(rope_half) + o, torch.arange(rope_half) + rope_half + o
        a, b = x[:, ia], x[:, ib]
        out[:, ia], out[:, ib] = (a * c - b * s).half(), (b * c + a * s).half()
    return out


# ---- emulations ------------------------------------------------------------------------------------------------------------

def flash_emulate(q, k, v, scale, rel_k=None, rel_v=None, kr=None, bq=16, stride=8, hi_inclusive=False, lo_early=False,
                  band_unmasked=False, hide=None):
    """CPU emulation of the flash construction (flash_attn64_tile<QT>, flash_rel96_f16_kernel<QT>, bq = 16 QT) on fp16
    q / k / v [H][T][D]: fp32 scores, 32-key chunks dealt to 4 partial online softmaxes (chunk c0 + w + 4 n to wave w, in rising
    order, c0 = the first chunk of the tile's key range), probabilities rounded to fp16 into the PV product with their fp32 sum
    as the denominator, K rows clamped to T - 1 and V zero beyond T, the band's biased logits set aside and weighted with rel_v
    in fp32 at the end, the LDS combine, fp16 output.  It follows the rounding points, not the MFMA summation order or __expf.
    Mutants: stride (8 -> 16: the chunk loop skips two chunks of every four per wave), hi_inclusive (j <= hi), lo_early
    (j >= lo - 1), band_unmasked (a band key outside the range keeps its biased score), hide = (i, j): key j hidden from query i."""
    assert q.dtype == torch.float16
    H, T, D = q.shape
    tpad = (T + CHUNK - 1) // CHUNK * CHUNK
    qf, kf, vf = q.float(), k.float(), v.float()
    kf = kf[:, torch.arange(tpad).clamp(max=T - 1)]
    vf = torch.cat([vf, torch.zeros(H, tpad - T, D)], dim=1)
    sc = torch.tensor(scale, dtype=torch.float32)
    s_all = (qf @ kf.transpose(1, 2)) * sc
    lo = kr[:, 0].long() if kr is not None else torch.zeros(T, dtype=torch.long)
    hi = kr[:, 1].long() if kr is not None else torch.full((T,), T, dtype=torch.long)
    mlo, mhi = lo - (1 if lo_early else 0), hi + (1 if hi_inclusive else 0)
    bias = (qf @ rel_k.float().t()) * sc if rel_k is not None else None
    out = torch.empty(T, H * D, dtype=torch.float16)
    for q0 in range(0, T, bq):
        q1 = min(q0 + bq, T)
        rows = torch.arange(q0, q1)
        nq = q1 - q0
        c0 = int(lo[q0]) >> 5 if kr is not None else 0
        nch = (int(hi[min(q0 + bq - 1, T - 1)]) + 31) >> 5 if kr is not None else tpad // CHUNK
        mw = torch.full((WAVES, H, nq), NINF)
        lw = torch.zeros(WAVES, H, nq)
        ow = torch.zeros(WAVES, H, nq, D)
        sb = torch.full((H, nq, NB), NINF)
        for w in range(WAVES):
            order, c = [], c0 + w
            while c < nch:
                order += [x for x in (c, c + 4) if x < nch]
                c += stride
            for cc in order:
                j = torch.arange(cc * CHUNK, (cc + 1) * CHUNK)
                m = (j[None, :] >= mlo[rows, None]) & (j[None, :] < mhi[rows, None])
                if hide is not None and q0 <= hide[0] < q1 and j[0] <= hide[1] <= j[-1]:
                    m[hide[0] - q0, hide[1] - int(j[0])] = False
                raw = s_all[:, q0:q1, j[0]:j[-1] + 1]
                s = raw.masked_fill(~m, NINF)
                if bias is not None:
                    r = j[None, :] - rows[:, None] + W
                    band = (r >= 0) & (r < NB) & (j[None, :] < tpad)
                    inb = band if band_unmasked else band & m
                    bsel = bias[:, q0:q1].gather(2, r.clamp(0, NB - 1).expand(H, nq, CHUNK))
                    s = torch.where(inb, raw + bsel, s)
                    ii, jj = torch.nonzero(inb, as_tuple=True)
                    sb[:, ii, r[ii, jj]] = s[:, ii, jj]
                mnew = torch.maximum(mw[w], s.max(-1).values)
                ms = torch.where(mnew == NINF, torch.zeros_like(mnew), mnew)
                alpha = torch.exp(mw[w] - ms)
                p = torch.exp(s - ms[..., None])
                lw[w] = lw[w] * alpha + p.sum(-1)
                mw[w] = mnew
                ow[w] = ow[w] * alpha[..., None] + p.half().float() @ vf[:, j[0]:j[-1] + 1]
        mt = mw.max(0).values
        e = torch.exp(mw - mt)
        den = (e * lw).sum(0)
        acc = (ow * e[..., None]).sum(0)
        if rel_v is not None:
            acc = acc + torch.exp(sb - mt[..., None]) @ rel_v.float()
        out[q0:q1] = merge((acc * (1.0 / den)[..., None]).half())
    return out


def mat_emulate(q, k, v, scale, rel_k=None, rel_v=None, kr=None):
    """CPU emulation of attention_mat<T> in the dtype of q: fp32 scores (GEMM, scaled in its epilogue), softmax_rows_kernel
    (bias on the band, range mask, fp32 max / exp / sum, p = e * (1 / sum), an empty range gives a zero row), P and V^T in the
    dtype, the PV GEMM with fp32 accumulation stored in the dtype, relv_add_kernel's re-read, fp32 add and second store"""
    dt = q.dtype
    H, Tq, _ = q.shape
    Tk = k.shape[1]
    sc = torch.tensor(scale, dtype=torch.float32)
    s = (q.float() @ k.float().transpose(1, 2)) * sc
    if rel_k is not None:
        r, band = _band_index(Tq, Tk)
        b = (q.float() @ rel_k.float().t()) * sc
        s = s + torch.where(band, b.gather(2, r.clamp(0, NB - 1).expand(H, Tq, Tk)), torch.zeros(()))
    vis = visible(kr, Tq, Tk)
    empty = ~vis.any(dim=1)
    s = s.masked_fill(~vis, NINF)
    s[:, empty] = 0.0
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    p = e * (1.0 / e.sum(-1, keepdim=True))
    p[:, empty] = 0.0
    out = (p.to(dt).float() @ v.float()).to(dt)
    if rel_v is not None:
        pb = torch.zeros(H, Tq, NB)
        i = torch.arange(Tq)
        for rr in range(NB):
            j = i + rr - W
            ok = (j >= 0) & (j < Tk)
            pb[:, i[ok], rr] = p[:, i[ok], j[ok]]
        out = (out.float() + pb @ rel_v.float()).to(dt)
    return merge(out)


# ---- refusals: what the hooks must refuse before any launch (dtype codes: GSV_F32 = 0, GSV_F16 = 1) ---------------------------
# rows hook: name, (qkv, vt, out) present, T, heads, rows, rope (table present), rope_half, qt, message
ROWS_REFUSALS = [
    ("null qkv", (0, 1, 1), 5, 2, 1, 0, 0, 0, "null pointer"),
    ("null vt", (1, 0, 1), 5, 2, 1, 0, 0, 0, "null pointer"),
    ("null out", (1, 1, 0), 5, 2, 1, 0, 0, 0, "null pointer"),
    ("T 0", (1, 1, 1), 0, 2, 1, 0, 0, 0, "bad shape"),
    ("rows 0", (1, 1, 1), 5, 2, 0, 0, 0, 0, "bad shape"),
    ("heads 0", (1, 1, 1), 5, 0, 1, 0, 0, 0, "bad shape"),
    ("qt 3", (1, 1, 1), 5, 2, 1, 0, 0, 3, "qt 3"),
    ("qt 8", (1, 1, 1), 5, 2, 1, 0, 0, 8, "qt 8"),
    ("qt -1", (1, 1, 1), 5, 2, 1, 0, 0, -1, "qt -1"),
    ("rope_half -1", (1, 1, 1), 5, 2, 1, 1, -1, 0, "rope_half -1"),
    ("rope_half past the projection", (1, 1, 1), 5, 2, 1, 1, 65, 0, "rope_half 65"),
    ("rope_half without a table", (1, 1, 1), 5, 2, 1, 0, 8, 0, "without a cos / sin table"),
]
# attention hook: name, (q, kv, out) present, Tq, Tk, heads, kc, rel (tables present), kr or None, dtype, route, message
ATTN_REFUSALS = [
    ("null q", (0, 1, 1), 5, 5, 2, 96, 1, None, 1, 0, "null pointer"),
    ("null kv", (1, 0, 1), 5, 5, 2, 96, 1, None, 1, 0, "null pointer"),
    ("null out", (1, 1, 0), 5, 5, 2, 96, 1, None, 1, 0, "null pointer"),
    ("dtype 2", (1, 1, 1), 5, 5, 2, 96, 1, None, 2, 0, "bad dtype"),
    ("route 3", (1, 1, 1), 5, 5, 2, 96, 1, None, 1, 3, "unknown route"),
    ("route -1", (1, 1, 1), 5, 5, 2, 96, 1, None, 1, -1, "unknown route"),
    ("Tq 0", (1, 1, 1), 0, 5, 2, 96, 0, None, 1, 2, "bad shape"),
    ("heads 0", (1, 1, 1), 5, 5, 0, 96, 0, None, 1, 2, "bad shape"),
    ("route 1 fp32", (1, 1, 1), 5, 5, 2, 96, 1, None, 0, 1, "fp16 only"),
    ("route 1 kc 64", (1, 1, 1), 5, 5, 2, 64, 1, None, 1, 1, "kc 96"),
    ("route 1 without tables", (1, 1, 1), 5, 5, 2, 96, 0, None, 1, 1, "needs rel_k and rel_v"),
    ("route 1 cross", (1, 1, 1), 5, 7, 2, 96, 1, None, 1, 1, "needs Tq == Tk"),
    ("one table", (1, 1, 1), 5, 5, 2, 96, 2, None, 1, 2, "come together"),
    ("range past Tk", (1, 1, 1), 3, 3, 2, 96, 1, [0, 3, 0, 4, 0, 3], 1, 2, "leaves [0, 3]"),
    ("range below 0", (1, 1, 1), 3, 3, 2, 96, 1, [-1, 3, 0, 3, 0, 3], 1, 2, "leaves [0, 3]"),
    ("range hi < lo", (1, 1, 1), 3, 3, 2, 96, 1, [0, 3, 2, 1, 0, 3], 1, 2, "leaves [0, 3]"),
    ("fused, lo descends", (1, 1, 1), 3, 3, 2, 96, 1, [1, 3, 0, 3, 0, 3], 1, 1, "descends"),
    ("fused, hi descends", (1, 1, 1), 3, 3, 2, 96, 1, [0, 3, 0, 2, 0, 3], 1, 1, "descends"),
    ("fused, empty range", (1, 1, 1), 3, 3, 2, 96, 1, [0, 3, 3, 3, 0, 3], 1, 1, "empty or descends"),
]
