"""GPU: gsv_op_align_logp / gsv_op_align_path / gsv_op_align (csrc/align.hip) against the host mirrors of _align_ref.py.

Shapes: nl in {1, 2, 63, 64, 65, 129, 1024} (1, 2, 3 and 16 phonemes per lane and both sides of a lane boundary; decision fields
of 1, 4 and 16 bits; decision bits in the LDS and, from 2051 x 1024 on, in the workspace) x nf in {nl, nl + 1, 2 nl + 3}, plus
nf = 400, nl = 57.  All spans of a test travel in ONE call, at odd row offsets of q [.][512] and k [.][1024] (ldk = 1024, the
engine's fused k|v rows).  nf < nl, nl = 1025 and empty spans take the fallback.

(a) the search on test-made fp32 lp (random, constant, quantised to 4 levels: ties everywhere): ends equal the float64 mirror and
    the score is bit-equal to it.
(b) the log-probabilities, f16 and f32 operands, against the fp64 mirror under the bar DERIVED in _align_ref.py for this kernel's
    summation: 2 gamma_{d+2} scale max sum|q_i k_i| + (nl + 4 max|s| + H + 16) 2^-24 + ulp32(|lp|).  The worst fraction is printed.
(c) both launches: the device path, scored under the mirror's fp64 lp, is within 2 nf bar of the mirror's optimum, for every
    shape; on planted inputs the ends are exactly the planted ones.
Nine spans of different sizes in one call are bit-equal (lp, ends, score) to each of them alone in a call."""
import ctypes as C

import numpy as np
import pytest
import torch

import _align_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, D = 4, 128
SCALE = 1.0 / np.sqrt(np.float32(D))
NLS = (1, 2, 63, 64, 65, 129, 1024)
SHAPES = [(nf, nl) for nl in NLS for nf in (nl, nl + 1, 2 * nl + 3)] + [(400, 57)]
FALLBACK = [(3, 5), (1030, 1025), (0, 0), (0, 5), (5, 0)]
NINE = [(400, 57), (65, 65), (131, 64), (129, 129), (261, 129), (7, 2), (1, 1), (3, 5), (2051, 1024)]


def _table(shapes, odd=True):
    """spans of `shapes` back to back, each starting at an odd row of q and of k; -> numpy table, q rows, k rows"""
    tab = np.zeros(len(shapes), np.dtype(_lib().ALIGN_SPAN_DTYPE))
    f = l = o = 0
    for i, (nf, nl) in enumerate(shapes):
        f += 1 if odd and f % 2 == 0 else 2 if odd else 0
        l += 1 if odd and l % 2 == 0 else 2 if odd else 0
        tab[i] = (f, nf, l, nl, o, 0)
        f, l, o = f + nf, l + nl, o + nl
    return tab, f + 1, l + 1


def _lib():
    from gsv import _lib as m
    return m


def _workspace(tab):
    m = _lib()
    offs = np.zeros(len(tab), np.int64)
    nbytes = m.lib().gsv_op_align_workspace(len(tab), tab.ctypes.data_as(C.POINTER(m.AlignSpan)), offs.ctypes.data_as(C.POINTER(C.c_int64)))
    assert nbytes > 0 and nbytes % 4 == 0 and (offs % 16 == 0).all()
    return nbytes, offs // 4


def _call(tab, q=None, k=None, lps=None, mode="align", ws_bytes=None):
    """one call of `mode` (logp / path / align) -> (lp per span or None, ends, score)"""
    m = _lib()
    m.init(0)
    l = m.lib()
    nbytes, offs = _workspace(tab)
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=DEV)
    if lps is not None:
        host = np.full(nbytes // 4, np.nan, np.float32)
        for sp, o, lp in zip(tab, offs, lps):
            if R.searched(int(sp["nf"]), int(sp["nl"])):
                host[o:o + lp.size] = lp.ravel()
        ws.copy_(torch.from_numpy(host))
    dtab = torch.from_numpy(tab.view(np.int32).reshape(len(tab), 6).copy()).to(DEV)
    n_out = int(tab["nl"].clip(min=0).sum())
    ends = torch.full((max(n_out, 1),), -7, dtype=torch.int32, device=DEV)
    score = torch.full((len(tab),), 123.0, dtype=torch.float32, device=DEV)
    wb = nbytes if ws_bytes is None else ws_bytes
    if mode != "path":
        dt = m.dtype_code(q.dtype)
        head = (q.data_ptr(), q.shape[1], k.data_ptr(), k.shape[1], dt, H, D, float(SCALE), dtab.data_ptr(), len(tab), ws.data_ptr(), wb)
    if mode == "logp":
        m.check(l.gsv_op_align_logp(*head, None), "gsv_op_align_logp")
    elif mode == "path":
        m.check(l.gsv_op_align_path(dtab.data_ptr(), len(tab), ws.data_ptr(), wb, ends.data_ptr(), score.data_ptr(), None), "gsv_op_align_path")
    else:
        m.check(l.gsv_op_align(*head, ends.data_ptr(), score.data_ptr(), None), "gsv_op_align")
    torch.cuda.synchronize()
    wsh, e, s = ws.cpu().numpy(), ends.cpu().numpy(), score.cpu().numpy()
    out_lp = [wsh[o:o + int(sp["nf"]) * int(sp["nl"])].reshape(int(sp["nf"]), int(sp["nl"])).copy()
              if R.searched(int(sp["nf"]), int(sp["nl"])) else None for sp, o in zip(tab, offs)]
    out_e = [e[int(sp["out0"]):int(sp["out0"]) + max(int(sp["nl"]), 0)].copy() for sp in tab]
    return out_lp, out_e, s


def _operands(tab, qrows, krows, dtype, seed):
    """random q (x 3: row maxima of the scores around 8) and k at the spans' rows, NaN elsewhere (a read outside a span shows)"""
    g = torch.Generator().manual_seed(seed)
    q = (3.0 * torch.randn(qrows, H * D, generator=g)).to(dtype)
    k = torch.randn(krows, 2 * H * D, generator=g).to(dtype)
    qm, km = torch.zeros(qrows, dtype=torch.bool), torch.zeros(krows, dtype=torch.bool)
    for sp in tab:
        qm[int(sp["f0"]):int(sp["f0"]) + int(sp["nf"])] = True
        km[int(sp["l0"]):int(sp["l0"]) + int(sp["nl"])] = True
    q[~qm] = float("nan")
    k[~km] = float("nan")
    return q, k


def _mirror(tab, q, k):
    out = []
    for sp in tab:
        nf, nl = int(sp["nf"]), int(sp["nl"])
        if not R.searched(nf, nl):
            out.append(None)
            continue
        qs = q[int(sp["f0"]):int(sp["f0"]) + nf].double().numpy()
        ks = k[int(sp["l0"]):int(sp["l0"]) + nl, :H * D].double().numpy()
        lp, a_max, s_max = R.logp_mirror(qs, ks, H, SCALE)
        out.append((lp, R.logp_bar(lp, a_max, s_max, H, D, SCALE)))
    return out


_cache = {}


def _logp_case(dtype):
    """the 22 shapes and the fallback spans in one gsv_op_align call; its operands, mirror and results, computed once per dtype"""
    if dtype not in _cache:
        tab, qrows, krows = _table(SHAPES + FALLBACK)
        q, k = _operands(tab, qrows, krows, dtype, seed=11)
        lp, ends, score = _call(tab, q.to(DEV), k.to(DEV), mode="align")
        _cache[dtype] = (tab, q, k, _mirror(tab, q, k), lp, ends, score)
    return _cache[dtype]


def _made_lp(nf, nl, kind, rng):
    if kind == "const":
        return np.full((nf, nl), -2.5, np.float32)
    x = rng.standard_normal((nf, nl)).astype(np.float32) * 3.0 - 4.0
    if kind == "quant4":
        return -np.floor(rng.random((nf, nl)) * 4.0).astype(np.float32)
    return x


@pytest.mark.parametrize("kind", ["random", "const", "quant4"])
def test_path_equals_the_float64_mirror(kind):
    rng = np.random.default_rng(5)
    shapes = SHAPES + FALLBACK
    tab, _, _ = _table(shapes)
    lps = [_made_lp(max(nf, 0), max(nl, 0), kind, rng) for nf, nl in shapes]
    _, ends, score = _call(tab, lps=lps, mode="path")
    for (nf, nl), lp, e, s in zip(shapes, lps, ends, score):
        if nf <= 0 or nl <= 0:
            assert s == -np.inf and (e == -7).all(), (nf, nl, "an empty span writes no ends")
            continue
        want, ws, _ = R.dp_mirror(lp)
        assert e.tolist() == want.tolist(), (kind, nf, nl)
        assert np.float32(s).tobytes() == np.float32(ws).tobytes(), (kind, nf, nl, s, ws)
        if R.searched(nf, nl):
            assert e[-1] == nf and e[0] >= 1 and (np.diff(e) >= 1).all()
        else:
            assert s == -np.inf


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_logp_within_the_derived_bar(dtype):
    tab, q, k, mir, lp, _, _ = _logp_case(dtype)
    worst = 0.0
    for sp, m, got in zip(tab, mir, lp):
        if m is None:
            assert got is None
            continue
        ref, bar = m
        assert np.isfinite(got).all(), (int(sp["nf"]), int(sp["nl"]))
        frac = float((np.abs(got.astype(np.float64) - ref) / bar).max())
        print(f"[align_logp] {str(dtype)[6:]} nf {int(sp['nf'])} nl {int(sp['nl'])}: largest |error| / bar = {frac:.3f} "
              f"(bar {bar.max():.2e})")
        worst = max(worst, frac)
    print(f"[align_logp] {str(dtype)[6:]}: worst fraction of the bar over {len(SHAPES)} shapes = {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_align_path_is_optimal_under_the_mirror(dtype):
    tab, q, k, mir, lp, ends, score = _logp_case(dtype)
    for sp, m, got, e, s in zip(tab, mir, lp, ends, score):
        nf, nl = int(sp["nf"]), int(sp["nl"])
        if nf <= 0 or nl <= 0:
            assert s == -np.inf
            continue
        if m is None:
            assert e.tolist() == R.fallback_ends(nf, nl).tolist() and s == -np.inf
            continue
        ref, bar = m
        _, _, V = R.dp_mirror(ref, keep64=True)
        loss = V[nl - 1] - R.path_sum(ref, e)
        assert loss <= 2.0 * nf * bar.max(), (nf, nl, loss, 2.0 * nf * bar.max())
        # and the two launches agree with each other: the path is the exact optimum of the lp the first launch wrote
        want, ws, _ = R.dp_mirror(got)
        assert e.tolist() == want.tolist() and np.float32(s).tobytes() == np.float32(ws).tobytes()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_planted_alignments_are_recovered(dtype):
    cases = [(400, 57), (131, 100), (64, 64), (9, 1), (300, 128)]
    tab, qrows, krows = _table(cases)
    q = torch.full((qrows, H * D), float("nan"))
    k = torch.full((krows, 2 * H * D), float("nan"))
    planted = []
    for sp, (nf, nl) in zip(tab, cases):
        qs, ks, scale, e = R.planted(nf, nl, H, D, seed=nf)
        q[int(sp["f0"]):int(sp["f0"]) + nf] = torch.from_numpy(qs) * float(np.sqrt(scale / SCALE))
        k[int(sp["l0"]):int(sp["l0"]) + nl, :H * D] = torch.from_numpy(ks) * float(np.sqrt(scale / SCALE))
        planted.append(e)
    # both operands carry the factor sqrt(scale / SCALE), so the true phoneme leads by about 4 in the scores whatever fp16 does to it
    _, ends, score = _call(tab, q.to(dtype).to(DEV), k.to(dtype).to(DEV), mode="align")
    for e, want, s in zip(ends, planted, score):
        assert e.tolist() == want.tolist()
        assert np.isfinite(s) and s <= 1e-4, "a mean log-probability: at most 0, up to the bar of lp (about 1e-5 on these operands)"


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_a_span_does_not_depend_on_its_neighbours(dtype):
    tab, qrows, krows = _table(NINE)
    q, k = _operands(tab, qrows, krows, dtype, seed=23)
    qd, kd = q.to(DEV), k.to(DEV)
    lp9, e9, s9 = _call(tab, qd, kd, mode="align")
    for i in range(len(NINE)):
        one = tab[i:i + 1].copy()
        one["out0"] = 0
        lp1, e1, s1 = _call(one, qd, kd, mode="align")
        assert (lp9[i] is None) == (lp1[0] is None)
        if lp9[i] is not None:
            assert lp9[i].tobytes() == lp1[0].tobytes(), NINE[i]
        assert e9[i].tobytes() == e1[0].tobytes() and s9[i:i + 1].tobytes() == s1.tobytes(), NINE[i]


def test_a_short_workspace_takes_the_fallback_and_bad_arguments_are_refused():
    m = _lib()
    tab, qrows, krows = _table([(7, 2), (400, 57)])
    q, k = _operands(tab, qrows, krows, torch.float16, seed=1)
    nbytes, offs = _workspace(tab)
    _, ends, score = _call(tab, q.to(DEV), k.to(DEV), mode="align", ws_bytes=int(offs[1]) * 4 + 64)
    assert np.isfinite(score[0]) and score[1] == -np.inf
    assert ends[1].tolist() == R.fallback_ends(400, 57).tolist()
    l = m.lib()
    qd, kd = q.to(DEV), k.to(DEV)
    dtab = torch.from_numpy(tab.view(np.int32).reshape(2, 6).copy()).to(DEV)
    ws = torch.zeros(nbytes // 4, device=DEV)
    args = lambda **kw: (qd.data_ptr(), kw.get("ldq", 512), kd.data_ptr(), 1024, m.GSV_F16, kw.get("heads", H), kw.get("hd", D),
                         kw.get("scale", 0.1), dtab.data_ptr(), kw.get("n", 2), ws.data_ptr(), nbytes, None)
    assert l.gsv_op_align_logp(*args()) == 0
    for bad in (dict(ldq=511), dict(heads=9), dict(hd=120), dict(scale=0.0), dict(n=0), dict(n=5000)):
        assert l.gsv_op_align_logp(*args(**bad)) != 0, bad
    assert l.gsv_op_align_workspace(-1, None, None) < 0
    torch.cuda.synchronize()
