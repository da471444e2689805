"""The AR prefill attention (csrc/t2s_prefill.hip) restated for the tests: the float64 mirror and its per-element bars, the
inputs of the three regimes, the table of shapes, and a CPU emulation of the fp16 flash kernel's arithmetic.

Rows are packed as the engine packs them: utterance b holds S_b = x_len[b] + p_len[b] rows [text | audio] of [q | k | v],
each d = 32 * H wide.  Mask (t2s_model.py:655-683): query i sees the keys j < (i < X ? X : i + 1).
"""
import math

import torch

HD = 32                      # head dim the kernels are built for
BQ, CHUNK, WAVES = 64, 32, 4   # prefill_flash32_f16_kernel<4>: queries per workgroup, keys per chunk, chunk c -> wave c % 4

# single-row shapes (X, P) on every side of the flash kernel's edges
SHAPES = [
    (1, 0), (1, 1),                       # one key; waves 1-3 own nothing
    (31, 0), (32, 0), (33, 0),            # text only around one chunk
    (15, 2), (16, 1),                     # text / audio boundary inside / at a 16-row sub-tile
    (37, 50),                             # boundary inside a chunk and inside a 64-query tile
    (63, 65), (64, 64), (65, 63),         # boundary around the query tile, S = 128: 4 chunks
    (100, 29),                            # S = 129: 5 chunks, only wave 0's second slot is valid
    (200, 56), (200, 57),                 # 8 / 9 chunks: the second trip of the loop first happens
    (300, 5), (5, 300),                   # all text with 10 chunks for every tile / almost purely causal
    (250, 390),                           # S = 640: 20 chunks, third trip, text tiles stop at X = 250
    (300, 0),                             # the uniform prompt-free entry
]
RAGGED = [(37, 50), (300, 5), (1, 1), (5, 300), (64, 64), (200, 57)]
REGIMES = ("flat", "sharp", "adversarial")
QK_SCALE = {"flat": 0.5, "sharp": 2.0, "adversarial": 2.0}


def row_offsets(x_len, p_len):
    off, m = [], 0
    for x, p in zip(x_len, p_len):
        off.append(m)
        m += x + p
    return off, m


def visible(X, P):
    """[S][S] bool: key j is visible to query i"""
    S = X + P
    i = torch.arange(S)
    lim = torch.where(i < X, torch.full_like(i, X), i + 1)
    return torch.arange(S)[None, :] < lim[:, None]


def _seed(x_len, p_len, H, regime, seed):
    s = 1000003 * seed + 7919 * REGIMES.index(regime) + 31 * H
    for x, p in zip(x_len, p_len):
        s = (s * 1315423911 + 2654435761 * x + 40503 * p + 17) % (2 ** 61 - 1)
    return s


def _make_row(X, P, H, regime, g):
    S, d = X + P, HD * H
    sc = QK_SCALE[regime]
    q = torch.randn(S, H, HD, generator=g) * sc
    k = torch.randn(S, H, HD, generator=g) * sc
    v = torch.rand(S, H, HD, generator=g) * 2 - 1
    if regime == "adversarial" and P > 0:
        # every query's largest raw score sits on its first invisible key: an off-by-one in the mask moves outputs by O(1)
        u = torch.randn(1, H, HD, generator=g) * sc
        q[:X] += u                                   # the text queries share a component, so one key can lead for all of them
        k[X] = 1.5 * q[:X].mean(0)                   # key X (first hidden key of every text query) pulled towards their mean
        k[X + 1:] = 1.5 * q[X:S - 1]                 # audio query i: key i + 1 is 1.5 q_i
    return torch.cat([q.reshape(S, d), k.reshape(S, d), v.reshape(S, d)], dim=1)


def make_qkv(x_len, p_len, H, regime, dtype, seed=0):
    """packed [M][3 d] rows of `dtype`; each utterance's values depend on its own (X, P, H, regime, seed) only, so a row of a
    ragged batch holds what the same row holds when it is launched alone"""
    rows = []
    for x, p in zip(x_len, p_len):
        g = torch.Generator().manual_seed(_seed([x], [p], H, regime, seed))
        rows.append(_make_row(x, p, H, regime, g))
    return torch.cat(rows, dim=0).to(dtype)


def _heads(qkv, H):
    S, d = qkv.shape[0], HD * H
    q, k, v = (qkv[:, c * d:(c + 1) * d].reshape(S, H, HD).transpose(0, 1) for c in range(3))
    return q, k, v   # [H][S][32]


def prefill_attn_ref(qkv, x_len, p_len, H, vis=None):
    """float64 mirror on the dtype-rounded values: ref = softmax(q k^T / sqrt(32) over the visible keys) v, and A = P |v|.
    vis: optional list of [S_b][S_b] bool masks replacing visible() (mutation tests)."""
    off, M = row_offsets(x_len, p_len)
    assert qkv.shape == (M, 3 * HD * H)
    ref = torch.empty(M, HD * H, dtype=torch.float64)
    A = torch.empty_like(ref)
    for b, (X, P) in enumerate(zip(x_len, p_len)):
        S = X + P
        q, k, v = _heads(qkv[off[b]:off[b] + S].double(), H)
        s = q @ k.transpose(1, 2) / math.sqrt(HD)
        m = visible(X, P) if vis is None else vis[b]
        p = torch.softmax(s.masked_fill(~m, -float("inf")), dim=-1)
        ref[off[b]:off[b] + S] = (p @ v).transpose(0, 1).reshape(S, -1)
        A[off[b]:off[b] + S] = (p @ v.abs()).transpose(0, 1).reshape(S, -1)
    return ref, A


def hidden_mass_fraction(qkv, x_len, p_len, H):
    """of the (query, head) pairs that have an invisible key: the fraction whose unmasked softmax puts >= 0.5 of its mass on
    the keys the mask hides"""
    off, _ = row_offsets(x_len, p_len)
    hit = tot = 0
    for b, (X, P) in enumerate(zip(x_len, p_len)):
        S = X + P
        q, k, _ = _heads(qkv[off[b]:off[b] + S].double(), H)
        p = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(HD), dim=-1)
        m = visible(X, P)
        has = ~m.all(dim=1)
        hidden = (p * (~m)).sum(-1)[:, has]
        hit += int((hidden >= 0.5).sum())
        tot += hidden.numel()
    return hit / tot if tot else 1.0


def _row_S(x_len, p_len):
    return torch.cat([torch.full((x + p,), float(x + p), dtype=torch.float64) for x, p in zip(x_len, p_len)])[:, None]


def flash_bar(ref, A, x_len, p_len):
    """fp16 output rounding + probabilities rounded to fp16 before the PV MFMA + subnormal probabilities"""
    return 2.0 ** -11 * ref.abs() + 2.0 ** -11 * A + _row_S(x_len, p_len) * 2.0 ** -25


def scalar_f16_bar(ref):
    """fp16 output rounding + the project's fp32 decode-attention tolerance for |v| <= 1"""
    return 2.0 ** -11 * ref.abs() + 2e-5


def scalar_f32_bar(ref):
    return torch.full_like(ref, 2e-5)


def route_bar(route, dtype, ref, A, x_len, p_len):
    if route in (1, 2):
        return flash_bar(ref, A, x_len, p_len)
    return scalar_f16_bar(ref) if dtype == torch.float16 else scalar_f32_bar(ref)


def check(out, ref, bar, what=""):
    """worst err / bar; AssertionError if an element lies outside its bar (or is not finite)"""
    o = out.double()
    assert torch.isfinite(o).all(), f"{what}: non-finite output"
    ratio = (o - ref).abs() / bar
    worst = float(ratio.max())
    if worst > 1.0:
        i = int(ratio.argmax())
        r, c = i // ref.shape[1], i % ref.shape[1]
        raise AssertionError(f"{what}: element [{r}, {c}] outside the bar: got {float(o[r, c])!r}, mirror {float(ref[r, c])!r}, "
                             f"bar {float(bar[r, c]):.3e}, err/bar {worst:.3f}; {int((ratio > 1).sum())} elements outside")
    return worst


def flash_emulate(qkv, x_len, p_len, H, vis=None):
    """CPU emulation of prefill_flash32_f16_kernel<4>'s construction on fp16 inputs: fp32 scores, 32-key chunks dealt to 4
    partial online softmaxes (chunk c to wave c % 4, in rising order), probabilities rounded to fp16 into the PV product with
    their fp32 sum as the denominator, K rows clamped to S - 1 and V zero beyond S, the LDS combine, fp16 output.
    vis: optional [S_b][ceil32(S_b)] bool masks replacing the kernel's `j < lim` (mutation tests)."""
    assert qkv.dtype == torch.float16
    off, M = row_offsets(x_len, p_len)
    out = torch.empty(M, HD * H, dtype=torch.float16)
    scale = torch.tensor(1.0 / math.sqrt(HD), dtype=torch.float32)
    ninf = -float("inf")
    for b, (X, P) in enumerate(zip(x_len, p_len)):
        S = X + P
        spad = (S + CHUNK - 1) // CHUNK * CHUNK
        q, k, v = _heads(qkv[off[b]:off[b] + S].float(), H)
        k = k[:, torch.arange(spad).clamp(max=S - 1)]
        v = torch.cat([v, torch.zeros(H, spad - S, HD)], dim=1)
        m_all = vis[b] if vis is not None else torch.cat([visible(X, P), torch.zeros(S, spad - S, dtype=torch.bool)], dim=1)
        s_all = (q @ k.transpose(1, 2)) * scale        # fp32 [H][S][spad]
        for q0 in range(0, S, BQ):
            q1 = min(q0 + BQ, S)
            nq = q1 - q0
            nk = X if q1 - 1 < X else q1
            nchunks = (nk + CHUNK - 1) // CHUNK
            mw = torch.full((WAVES, H, nq), ninf)
            lw = torch.zeros(WAVES, H, nq)
            ow = torch.zeros(WAVES, H, nq, HD)
            for c in range(nchunks):
                w, ks = c % WAVES, slice(c * CHUNK, (c + 1) * CHUNK)
                s = s_all[:, q0:q1, ks].masked_fill(~m_all[q0:q1, ks], ninf)
                mnew = torch.maximum(mw[w], s.max(-1).values)
                ms = torch.where(mnew == ninf, torch.zeros_like(mnew), mnew)
                alpha = torch.exp(mw[w] - ms)
                p = torch.exp(s - ms[..., None])
                lw[w] = lw[w] * alpha + p.sum(-1)
                mw[w] = mnew
                ow[w] = ow[w] * alpha[..., None] + p.half().float() @ v[:, ks]
            mt = mw.max(0).values
            e = torch.exp(mw - mt)
            den = (e * lw).sum(0)
            acc = (ow * e[..., None]).sum(0)
            out[off[b] + q0:off[b] + q1] = (acc / den[..., None]).half().transpose(0, 1).reshape(nq, -1)
    return out


# what gsv_op_prefill_attn must refuse before any launch (dtype codes: GSV_F32 = 0, GSV_F16 = 1)
REFUSALS = [   # name, (qkv, kc, vc, out) present, x_len, p_len, H, d, smax, dtype code, route, message
    ("null qkv", (0, 1, 1, 1), [5], [3], 2, 64, 16, 1, 3, "null pointer"),
    ("null kc", (1, 0, 1, 1), [5], [3], 2, 64, 16, 1, 3, "null pointer"),
    ("null vc", (1, 1, 0, 1), [5], [3], 2, 64, 16, 1, 3, "null pointer"),
    ("null out", (1, 1, 1, 0), [5], [3], 2, 64, 16, 1, 3, "null pointer"),
    ("d != 32 H", (1, 1, 1, 1), [5], [3], 2, 128, 16, 1, 3, "32 * H"),
    ("empty text", (1, 1, 1, 1), [5, 0], [3, 3], 2, 64, 16, 1, 3, "row 1"),
    ("negative prompt", (1, 1, 1, 1), [5, 5], [-1, 3], 2, 64, 16, 1, 3, "row 0"),
    ("S + 2 > smax", (1, 1, 1, 1), [5, 6], [3, 9], 2, 64, 16, 1, 3, "row 1"),
    ("route 1 fp32", (1, 1, 1, 1), [5], [3], 2, 64, 16, 0, 1, "fp16 only"),
    ("route 2 fp32", (1, 1, 1, 1), [5], [3], 2, 64, 16, 0, 2, "fp16 only"),
    ("route 4", (1, 1, 1, 1), [5], [3], 2, 64, 16, 1, 4, "unknown route"),
    ("route -1", (1, 1, 1, 1), [5], [3], 2, 64, 16, 1, -1, "unknown route"),
]
