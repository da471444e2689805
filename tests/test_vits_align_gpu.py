"""GPU: the phoneme alignment inside the SoVITS engine (gsv_vits_set_align; SynthesizerTrn.decode / decode_segments /
SynthesizerTrnV3.decode_encp with align=), small synthetic v2 and v3 models in fp32 and fp16.

- the waveform / features with align= are bit-equal to the call without;
- last_alignment is what gsv_op_align computes on the engine's own m_q / m_kv (debug tensors), bit for bit;
- fp32: the path, scored under log-probabilities rebuilt on the CPU with the oracle's enc_p chain up to the MRTE's q and k, is
  within 2 nf bar of that mirror's optimum, the bar (tests/_align_ref.py) evaluated on the oracle's operands;
- decode_segments, 3 segments of different voices, one at speed 1.25 and one holding two sentence spans: each span's path, scored
  under the mirror of that segment's own plain decode, is within 2 nf bar of its optimum;
- a pending table is consumed by exactly one call; spans outside their segment or sharing a phoneme are refused."""
import math

import numpy as np
import pytest
import torch

import _align_ref as R
from oracle import cases
from oracle.vits_oracle import VitsOracle
from test_align_op_gpu import _call, _table
from test_cfm_gpu import _v3
from test_vits_segments_gpu import DEV, _engine, _seg_inputs, _voice

pytestmark = pytest.mark.gpu
H, D = 4, 128
SCALE = 1.0 / np.sqrt(np.float32(D))


def _operands(m, T, L):
    """the MRTE attention's q [2T][512] and k|v [L][1024] of the last enc_p, in the engine's dtype"""
    q = m.debug_tensor("m_q", 512 * 2 * T).view(512, 2 * T).t().contiguous().to(m.dtype)
    kv = m.debug_tensor("m_kv", 1024 * L).view(1024, L).t().contiguous().to(m.dtype)
    return q, kv


def _op_on(m, T, L, spans):
    """gsv_op_align on the engine's operands for spans (code0, n_codes, phone0, n_phones)"""
    q, kv = _operands(m, T, L)
    tab = np.zeros(len(spans), np.dtype([(n, "<i4") for n in ("f0", "nf", "l0", "nl", "out0", "reserved")]))
    o = 0
    for i, (c0, nc, p0, npn) in enumerate(spans):
        tab[i] = (2 * c0, 2 * nc, p0, npn, o, 0)
        o += npn
    _, ends, score = _call(tab, q, kv, mode="align")
    return ends, score, q, kv


def _oracle_qk(sd, cfg, codes, text):
    """the MRTE attention's q [2T][512] and k [L][512] rebuilt on the CPU: the oracle's enc_p chain up to _mrte's projections"""
    vo = VitsOracle(sd, cfg)
    qo = sd["quantizer.vq.layers.0._codebook.embed"][codes[0, 0].cpu().long()].t().repeat_interleave(2, dim=1)
    y = vo._encoder(vo.conv(qo, "enc_p.ssl_proj"), "enc_p.encoder_ssl", vo.n_layers // 2)
    t = vo._encoder(sd["enc_p.text_embedding.weight"][text[0].cpu().long()].t(), "enc_p.encoder_text", vo.n_layers)
    p = "enc_p.mrte"
    qq = vo.conv(vo.conv(y, p + ".c_pre"), p + ".cross_attention.conv_q").t().double().numpy()
    kk = vo.conv(vo.conv(t, p + ".text_pre"), p + ".cross_attention.conv_k").t().double().numpy()
    return qq, kk


def _within(ends, q, k, what):
    lp, a_max, s_max = R.logp_mirror(q, k, H, SCALE)
    bar = R.logp_bar(lp, a_max, s_max, H, D, SCALE).max()
    nf, nl = lp.shape
    _, _, V = R.dp_mirror(lp, keep64=True)
    loss = V[nl - 1] - R.path_sum(lp, ends)
    print(f"[vits_align] {what}: nf {nf} nl {nl} loss {loss:.3e} of 2 nf bar {2 * nf * bar:.3e}")
    assert loss <= 2 * nf * bar, (what, loss, 2 * nf * bar)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_v2_decode_alignment(dtype):
    m, cfg, sd = _engine("small", dtype)
    T, L = 37, 23
    codes, text = _seg_inputs(T, L, "al0")
    v = _voice(1)
    ref = m.decode(codes, text, v[0], seed=77)
    m.last_alignment = None
    spans = [(0, 20, 0, 11), (20, 17, 11, 12)]
    out = m.decode(codes, text, v[0], seed=77, align=spans)
    assert torch.equal(out, ref), "the waveform does not depend on align="
    got = m.last_alignment
    assert len(got) == 2 and [len(e) for e, _ in got] == [11, 12]
    ends, score, q, kv = _op_on(m, T, L, spans)
    for (e, s), oe, os_ in zip(got, ends, score):
        assert e.tolist() == oe.tolist() and np.float32(s).tobytes() == np.float32(os_).tobytes()
        assert e[0] >= 1 and (np.diff(e) >= 1).all() and np.isfinite(s)
    assert got[0][0][-1] == 40 and got[1][0][-1] == 34
    # align=True: one span over everything
    m.decode(codes, text, v[0], seed=77, align=True)
    (e, s), = m.last_alignment
    oe, os_, _, _ = _op_on(m, T, L, [(0, T, 0, L)])
    assert e.tolist() == oe[0].tolist() and len(e) == L and e[-1] == 2 * T
    if dtype == torch.float32:
        qq, kk = _oracle_qk(sd, cfg, codes, text)
        assert qq.shape == (2 * T, 512) and kk.shape == (L, 512)
        _within(e, qq, kk, "v2 fp32 against the oracle's operands")
        for (es, _), (c0, nc, p0, npn) in zip(got, spans):
            _within(es, qq[2 * c0:2 * (c0 + nc)], kk[p0:p0 + npn], "v2 fp32 span against the oracle's operands")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_v3_decode_encp_alignment(dtype):
    case = cases.ENCP_CASES[sorted(cases.ENCP_CASES)[0]]
    cfg, sd, codes, text, refer = cases.encp_case_inputs(case)
    m = _v3(cfg, sd, case["version"], dtype)
    T, L = int(codes.shape[-1]), int(text.shape[-1])
    fea, ge = m.decode_encp(codes.to(DEV), text.to(DEV), refer.to(DEV), speed=case["speed"])
    assert m.last_alignment is None
    fea2, _ = m.decode_encp(codes.to(DEV), text.to(DEV), refer.to(DEV), ge=ge, speed=case["speed"], align=True)
    assert torch.equal(fea, fea2), "the features do not depend on align="
    (e, s), = m.last_alignment
    oe, os_, q, kv = _op_on(m, T, L, [(0, T, 0, L)])
    assert e.tolist() == oe[0].tolist() and np.float32(s).tobytes() == np.float32(os_[0]).tobytes()
    if 2 * T >= L:
        assert len(e) == L and e[-1] == 2 * T and (np.diff(e) >= 1).all()
        _within(e, q.double().cpu().numpy(), kv[:, :512].double().cpu().numpy(), f"v3 {dtype} against the engine's operands")
        if dtype == torch.float32:
            qq, kk = _oracle_qk(sd, cfg, codes, text)
            assert qq.shape == (2 * T, 512) and kk.shape == (L, 512)
            _within(e, qq, kk, "v3 fp32 against the oracle's operands")
    else:
        assert s == -np.inf and e.tolist() == R.fallback_ends(2 * T, L).tolist()


def test_segments_equal_each_segments_own_decode():
    m, cfg, sd = _engine("small", torch.float32)
    TL = [(19, 13), (31, 22), (11, 9)]
    speeds = [1.0, 1.25, 1.0]
    segs = [(*_seg_inputs(T, L, f"alseg{i}"), _voice(i), 300 + i) for i, (T, L) in enumerate(TL)]
    align = [True, [(0, 14, 0, 10), (14, 17, 10, 12)], True]
    args = ([s[0] for s in segs], [s[1] for s in segs], [s[2] for s in segs], [s[3] for s in segs])
    ref = m.decode_segments(*args, speeds=speeds)
    out = m.decode_segments(*args, speeds=speeds, align=align)
    assert all(torch.equal(a, b) for a, b in zip(out, ref)), "the waveforms do not depend on align="
    got = m.last_alignment
    assert [len(e) for e, _ in got] == [13, 10, 12, 9]
    assert [int(e[-1]) for e, _ in got] == [38, 28, 34, 22], "frames of the 50-per-second pre-speed axis, whatever the speed"
    r = 0
    for (codes, text, voice, seed), (T, L), al, spd in zip(segs, TL, align, speeds):
        spans = [(0, T, 0, L)] if al is True else al
        m.decode(codes, text, voice[0], seed=seed, speed=spd, align=spans)
        alone = m.last_alignment
        q, kv = _operands(m, T, L)
        qn, kn = q.double().cpu().numpy(), kv[:, :512].double().cpu().numpy()
        for (c0, nc, p0, npn), (ea, sa) in zip(spans, alone):
            es, ss = got[r]
            r += 1
            assert len(es) == len(ea) == npn and np.isfinite(ss) and np.isfinite(sa)
            _within(es, qn[2 * c0:2 * (c0 + nc)], kn[p0:p0 + npn], f"segmented span {r - 1}")
            _within(ea, qn[2 * c0:2 * (c0 + nc)], kn[p0:p0 + npn], f"plain span {r - 1}")
    assert r == 4


def test_a_pending_table_is_consumed_by_exactly_one_call_and_bad_spans_are_refused():
    m, cfg, sd = _engine("small", torch.float32)
    T, L = 12, 9
    codes, text = _seg_inputs(T, L, "al1")
    v = _voice(2)
    with torch.cuda.device(DEV):
        counts, ends, score = m._align_begin([(0, 0, T, 0, L)])
    m.decode(codes, text, v[0], seed=1)
    first = ends.cpu().numpy().copy()
    assert first[-1] == 2 * T and (np.diff(first) >= 1).all()
    ends.zero_()
    score.fill_(5.0)
    torch.cuda.synchronize()
    m.decode(codes, text, v[0], seed=1)
    assert (ends.cpu().numpy() == 0).all() and float(score[0]) == 5.0, "the second call found nothing pending"
    for bad in ([(0, T + 1, 0, L)], [(0, T, 1, L)], [(-1, 2, 0, 2)], [(0, T, 0, 5), (0, T, 4, 5)],
                [(0, T, 0, 6), (0, T, 3, 0), (0, T, 4, 5)]):          # an empty span between two that share phonemes
        with pytest.raises(RuntimeError):
            m.decode(codes, text, v[0], seed=1, align=bad)
    m.decode(codes, text, v[0], seed=1, align=[(0, T, 0, 5), (0, T, 5, 4)])        # the same frames for two phoneme runs is fine
    assert [len(e) for e, _ in m.last_alignment] == [5, 4]
    m.decode(codes, text, v[0], seed=1, align=[(0, T, 0, 5), (0, T, 2, 0), (0, T, 5, 4)])      # an empty span shares nothing
    assert [len(e) for e, _ in m.last_alignment] == [5, 0, 4]
    m.decode(codes, text, v[0], seed=1, align=[])
    assert m.last_alignment == [], "asked for with no span: not the result of the call before"
    with pytest.raises(RuntimeError):
        m.decode_segments([codes], [text], [v], [1], align=[[(0, T, 0, L + 1)]])
    ref = m.decode(codes, text, v[0], seed=1)
    assert torch.isfinite(ref).all(), "a refused table leaves the engine usable, with nothing pending"
