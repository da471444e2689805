"""GPU: the segmented SoVITS decode (SynthesizerTrn.decode_segments / gsv_vits_decode_segments).  Several sequences, each
with its own voice, seed and lengths, share one pass of enc_p, flow and generator; each must come out as its own
`decode` would produce it, and nothing may leak across a segment boundary."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from gsv import synthetic as S
from oracle import cases
from oracle.vits_oracle import VitsOracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_ENGINES = {}


def _cfg(name):
    if name == "small":
        return S.small_vits_config()
    if name == "v2":
        return S.VITS_V2_CONFIG
    cfg = copy.deepcopy(S.small_vits_config())                     # v2Pro as in oracle/cases.py
    cfg["model"]["version"] = "v2Pro"
    cfg["model"]["gin_channels"] = 1024
    return cfg


def _engine(cname, dtype, seed=3):
    key = (cname, dtype, seed)
    if key not in _ENGINES:
        from gsv.module.models import SynthesizerTrn
        cfg = _cfg(cname)
        d, mk = cfg["data"], dict(cfg["model"])
        version = mk.pop("version", "v2")
        sd = S.make_vits_state_dict(cfg, seed=seed)
        m = SynthesizerTrn(d["filter_length"] // 2 + 1, cfg["train"]["segment_size"] // d["hop_length"],
                           n_speakers=d["n_speakers"], version=version, device=DEV, dtype=dtype,
                           n_symbols=cfg["n_symbols"], **mk)
        m.load_state_dict(sd)
        _ENGINES[key] = (m, cfg, sd)
    return _ENGINES[key]


def _voice(i, pro=False, tr=None):
    tr = tr or 17 + 5 * (i % 4)
    refer = torch.from_numpy(S.hash_uniform(f"seg_refer{i}", 1025 * tr, 11).reshape(1, 1025, tr).copy()).to(DEV)
    sv = S.hash_symmetric(f"seg_sv{i}", (1, 20480), 1.0, 11).to(DEV) if pro else None
    return (refer, sv)


def _seg_inputs(T, L, tag, n_symbols=732):
    codes = torch.from_numpy(S.hash_ints(f"seg_codes_{tag}", T, 1024, 5)).view(1, 1, -1).to(DEV)
    text = torch.from_numpy(S.hash_ints(f"seg_text_{tag}", L, n_symbols, 5)).view(1, -1).to(DEV)
    return codes, text


def _alone(m, codes, text, voice, seed, noise=None):
    return m.decode(codes, text, voice[0], sv_emb=voice[1], noise=noise, seed=seed).float()


@pytest.mark.parametrize("cname", ["v2", "small", "v2pro"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_one_segment_is_the_plain_decode(cname, dtype):
    m, cfg, _ = _engine(cname, dtype)
    codes, text = _seg_inputs(200 if cname == "v2" else 37, 41, "one")
    v = _voice(0, pro=cname == "v2pro")
    ref = _alone(m, codes, text, v, 1234)
    out = m.decode_segments([codes], [text], [v], [1234])
    assert len(out) == 1 and out[0].shape == ref.shape
    assert torch.equal(out[0].float(), ref)


CODE_LENS = [1, 7, 37, 100, 203, 64]
PHONE_LENS = [3, 11, 23, 40, 9, 17]


def _six(m, pro=False, swap2=False):
    segs = []
    for i, (T, L) in enumerate(zip(CODE_LENS, PHONE_LENS)):
        tag = f"six{i}" + ("x" if (swap2 and i == 2) else "")
        codes, text = _seg_inputs(T, L, tag)
        vi = i % 3 if not (swap2 and i == 2) else 7
        segs.append((codes, text, _voice(vi, pro), 100 + i))
    return segs


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_no_leakage_across_segments(dtype):
    m, _, _ = _engine("small", dtype)
    outs = []
    for swap in (False, True):
        segs = _six(m, swap2=swap)
        outs.append(m.decode_segments([s[0] for s in segs], [s[1] for s in segs], [s[2] for s in segs], [s[3] for s in segs]))
    for i in range(6):
        if i != 2:
            assert torch.equal(outs[0][i], outs[1][i]), f"segment {i} changed when segment 2 changed"
    assert not torch.equal(outs[0][2], outs[1][2])


@pytest.mark.parametrize("cname", ["small", "v2pro"])
def test_each_segment_equals_its_isolated_decode_fp32(cname):
    pro = cname == "v2pro"
    m, cfg, sd = _engine(cname, torch.float32)
    segs = _six(m, pro=pro)
    IC = cfg["model"]["inter_channels"]
    noise = [S.hash_normal(f"seg_noise{i}", (IC, 2 * T), 9) for i, T in enumerate(CODE_LENS)]
    out = m.decode_segments([s[0] for s in segs], [s[1] for s in segs], [s[2] for s in segs], [s[3] for s in segs])
    outn = m.decode_segments([s[0] for s in segs], [s[1] for s in segs], [s[2] for s in segs], [s[3] for s in segs],
                             noise=noise)
    orc = VitsOracle(sd, cfg)
    for i, (codes, text, v, seed) in enumerate(segs):
        ref = _alone(m, codes, text, v, seed)
        assert out[i].shape == ref.shape
        assert (out[i].float() - ref).abs().max().item() <= 1e-5, f"segment {i}"
        refn = _alone(m, codes, text, v, seed, noise=noise[i])
        assert (outn[i].float() - refn).abs().max().item() <= 1e-5, f"segment {i} (explicit noise)"
        o = orc.decode(codes.cpu(), text.cpu(), [v[0].cpu()], noise=noise[i],
                       sv_emb=[v[1].cpu()] if pro else None).float()
        assert (outn[i].float().cpu() - o).abs().max().item() <= 1e-4, f"segment {i} vs oracle"


def test_production_shape_fp16():
    m16, cfg, sd = _engine("v2", torch.float16)
    m32, _, _ = _engine("v2", torch.float32)
    n, T = 32, 100
    segs = []
    for i in range(n):
        codes, text = _seg_inputs(T, 20 + (i * 7) % 31, f"prod{i}")
        segs.append((codes, text, _voice(100 + i, tr=20 + i), 7000 + i))
    IC = cfg["model"]["inter_channels"]
    noise = [S.hash_normal(f"prod_noise{i}", (IC, 2 * T), 9) for i in range(n)]
    out = m16.decode_segments([s[0] for s in segs], [s[1] for s in segs], [s[2] for s in segs], [s[3] for s in segs],
                              noise=noise)
    orc = VitsOracle(sd, cfg)
    for i, (codes, text, v, seed) in enumerate(segs):
        ref = _alone(m32, codes, text, v, seed, noise=noise[i])
        err = out[i].float() - ref
        assert err.abs().max().item() <= 2e-2, f"segment {i}"
        assert (err.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item() <= 0.03, f"segment {i}"
        if i in (0, 9, 22, 31):
            o = orc.decode(codes.cpu(), text.cpu(), [v[0].cpu()], noise=noise[i]).float()
            e = out[i].float().cpu() - o
            assert e.abs().max().item() <= 2e-2 and (e.pow(2).mean().sqrt() / o.pow(2).mean().sqrt()).item() <= 0.03


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_gap_rows_are_zero(dtype):
    from gsv import _lib
    m, cfg, _ = _engine("small", dtype)
    segs = _six(m)
    m.decode_segments([s[0] for s in segs], [s[1] for s in segs], [s[2] for s in segs], [s[3] for s in segs])
    mc = cfg["model"]
    vc = _lib.VitsConfig()
    vc.kernel_size = mc["kernel_size"]
    vc.n_ups = len(mc["upsample_rates"])
    for i, (u, k) in enumerate(zip(mc["upsample_rates"], mc["upsample_kernel_sizes"])):
        vc.up_rates[i], vc.up_kernels[i] = u, k
    vc.n_resblocks = len(mc["resblock_kernel_sizes"])
    for j, (k, ds) in enumerate(zip(mc["resblock_kernel_sizes"], mc["resblock_dilation_sizes"])):
        vc.rb_kernels[j] = k
        for c, d in enumerate(ds):
            vc.rb_dilations[j][c] = d
    n = len(CODE_LENS)
    cl, pl = (C.c_int * n)(*CODE_LENS), (C.c_int * n)(*PHONE_LENS)

    def seg_map(level):
        rows = C.c_int64(0)
        _lib.check(_lib.lib().gsv_vits_segment_map(C.byref(vc), n, cl, pl, level, None, 0, C.byref(rows)))
        buf = (C.c_int32 * rows.value)()
        _lib.check(_lib.lib().gsv_vits_segment_map(C.byref(vc), n, cl, pl, level, buf, rows.value, C.byref(rows)))
        return np.frombuffer(buf, dtype=np.int32).copy()

    IC = mc["inter_channels"]
    sf = seg_map(0)
    z = m.debug_tensor("z", IC * len(sf)).cpu().numpy().reshape(IC, len(sf))
    assert (sf < 0).sum() == (n - 1) * _lib.lib().gsv_vits_segment_gap(C.byref(vc))
    assert np.all(z[:, sf < 0] == 0) and np.abs(z[:, sf >= 0]).max() > 0
    last = vc.n_ups - 1
    sl = seg_map(last)
    ch = 2 * (mc["upsample_initial_channel"] >> vc.n_ups)
    g = m.debug_tensor("gen_last_in", ch * len(sl)).cpu().numpy().reshape(ch, len(sl))
    assert np.all(g[:, sl < 0] == 0) and np.abs(g[:, sl >= 0]).max() > 0


def test_errors_do_not_crash():
    from gsv import _lib
    m, _, _ = _engine("small", torch.float32)
    codes, text = _seg_inputs(5, 4, "err")
    m.decode_segments([codes], [text], [_voice(0)], [1])                       # stores slot 0
    l = _lib.lib()
    cd = codes.reshape(-1).to(torch.int32).contiguous()
    tx = text.reshape(-1).to(torch.int32).contiguous()
    wav = torch.empty(10 * 64 * 16, device=DEV)

    def call(code_lens, phone_lens, slots):
        n = len(code_lens)
        return l.gsv_vits_decode_segments(m._h, n, cd.data_ptr(), (C.c_int * n)(*code_lens), tx.data_ptr(),
                                          (C.c_int * n)(*phone_lens), (C.c_int * n)(*slots), (C.c_uint64 * n)(*([0] * n)),
                                          None, 0.5, wav.data_ptr(), None)

    assert call([5], [4], [77]) != 0 and b"slot" in l.gsv_last_error()        # a slot that holds no voice
    assert call([5], [4], [500]) != 0
    assert call([5, 0], [2, 2], [0, 0]) != 0 and b"empty" in l.gsv_last_error()
    assert l.gsv_vits_store_voice(m._h, 128) != 0
    torch.cuda.synchronize()
    assert call([5], [4], [0]) == 0                                            # the handle still works
    torch.cuda.synchronize()
    cfg3 = _lib.VitsConfig()                                                   # a v3 handle (no weights needed)
    cfg3.inter_channels = cfg3.hidden_channels = 192
    cfg3.n_heads, cfg3.flavor = 2, 1
    h3 = C.c_void_p()
    _lib.check(l.gsv_vits_create(C.byref(cfg3), 0, C.byref(h3)))
    try:
        rc = l.gsv_vits_decode_segments(h3, 1, cd.data_ptr(), (C.c_int * 1)(5), tx.data_ptr(), (C.c_int * 1)(4),
                                        (C.c_int * 1)(0), (C.c_uint64 * 1)(0), None, 0.5, wav.data_ptr(), None)
        assert rc != 0 and b"v3" in l.gsv_last_error()
    finally:
        l.gsv_vits_destroy(h3)
