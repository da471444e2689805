"""GPU: the segmented SoVITS decode with per-segment speeds (SynthesizerTrn.decode_segments(speeds=...) /
gsv_vits_decode_segments_speed).  Each segment is interpolated from its own frames to F_s frames after enc2, so each must
come out as its own `decode(speed=...)` would produce it -- slowed down, sped up to one frame, or left alone between two
others -- and nothing may leak across a segment boundary in either layout."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from gsv import synthetic as S
from oracle import cases
from oracle.vits_oracle import VitsOracle
from test_vits_segments_gpu import DEV, PHONE_LENS, _engine, _seg_inputs, _voice

pytestmark = pytest.mark.gpu

# slow-down next to a gap (i1 clamps at the right edge), one frame (shorter than every conv's reach), an exact quotient,
# a speed-1 segment between two others, the oracle's speed case, another slow-down at the end
CODE_LENS = [1, 1, 6, 37, 11, 5]
SPEEDS = [0.5, 3.0, 1.5, 1.0, 1.3, 0.8]
FRAMES = [5, 1, 9, 74, 17, 13]


def _alone(m, codes, text, voice, seed, speed, noise=None):
    return m.decode(codes, text, voice[0], sv_emb=voice[1], noise=noise, seed=seed, speed=speed).float()


def _six(pro=False, swap2=False):
    segs = []
    for i, (T, L) in enumerate(zip(CODE_LENS, PHONE_LENS)):
        tag = f"spd{i}" + ("x" if (swap2 and i == 2) else "")
        codes, text = _seg_inputs(T, L, tag)
        vi = i % 3 if not (swap2 and i == 2) else 7
        segs.append((codes, text, _voice(vi, pro), 200 + i))
    return segs


def _run(m, segs, **kw):
    return m.decode_segments([s[0] for s in segs], [s[1] for s in segs], [s[2] for s in segs], [s[3] for s in segs], **kw)


@pytest.mark.parametrize("cname", ["small", "v2pro"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("speed", [1.3, 0.8])
def test_one_segment_is_the_plain_decode(cname, dtype, speed):
    m, cfg, _ = _engine(cname, dtype)
    codes, text = _seg_inputs(37, 41, "one")
    v = _voice(0, pro=cname == "v2pro")
    ref = _alone(m, codes, text, v, 1234, speed)
    out = m.decode_segments([codes], [text], [v], [1234], speeds=[speed])
    assert len(out) == 1 and out[0].shape == ref.shape
    assert out[0].shape[-1] == (int(74 / speed) + 1) * math.prod(cfg["model"]["upsample_rates"])
    assert torch.equal(out[0].float(), ref)


def test_one_segment_matches_the_reference_golden():
    """T=11, L=7, speed 1.3 with the case's noise: the reference's waveform (golden of oracle case vits_small_speed)"""
    from gsv.module.models import SynthesizerTrn
    case = cases.VITS_CASES["vits_small_speed"]
    cfg, sd, codes, text, refers, noise, _ = cases.vits_case_inputs(case)
    assert codes.shape[-1] == 11 and text.shape[-1] == 7 and case["speed"] == 1.3
    g = load_golden("vits_small_speed")
    d, mk = cfg["data"], dict(cfg["model"])
    version = mk.pop("version", "v2")
    m = SynthesizerTrn(d["filter_length"] // 2 + 1, cfg["train"]["segment_size"] // d["hop_length"],
                       n_speakers=d["n_speakers"], version=version, device=DEV, dtype=torch.float32,
                       n_symbols=cfg["n_symbols"], **mk)
    m.load_state_dict(sd)
    voice = ([r.to(DEV) for r in refers], None)
    out = m.decode_segments([codes.to(DEV)], [text.to(DEV)], [voice], [0], noise_scale=case["noise_scale"], noise=[noise],
                            speeds=[1.3])
    assert tuple(out[0].shape) == g["wav"].shape
    err = np.abs(out[0].float().cpu().numpy() - g["wav"]).max()
    print(f"one segment at speed 1.3 vs reference golden: max-abs {err:.3e}")
    assert err <= 1e-4


@pytest.mark.parametrize("cname", ["small", "v2pro"])
def test_each_segment_equals_its_isolated_decode_fp32(cname):
    pro = cname == "v2pro"
    m, cfg, sd = _engine(cname, torch.float32)
    up = math.prod(cfg["model"]["upsample_rates"])
    segs = _six(pro=pro)
    IC = cfg["model"]["inter_channels"]
    noise = [S.hash_normal(f"spd_noise{i}", (IC, f), 9) for i, f in enumerate(FRAMES)]
    out = _run(m, segs, speeds=SPEEDS)
    outn = _run(m, segs, speeds=SPEEDS, noise=noise)
    orc = VitsOracle(sd, cfg)
    for i, (codes, text, v, seed) in enumerate(segs):
        ref = _alone(m, codes, text, v, seed, SPEEDS[i])
        assert ref.shape[-1] == FRAMES[i] * up, f"segment {i}: decode returns {ref.shape[-1] // up} frames"
        assert out[i].shape == ref.shape and outn[i].shape == ref.shape
        e = (out[i].float() - ref).abs().max().item()
        refn = _alone(m, codes, text, v, seed, SPEEDS[i], noise=noise[i])
        en = (outn[i].float() - refn).abs().max().item()
        o = orc.decode(codes.cpu(), text.cpu(), [v[0].cpu()], noise=noise[i], speed=SPEEDS[i],
                       sv_emb=[v[1].cpu()] if pro else None).float()
        eo = (outn[i].float().cpu() - o).abs().max().item()
        print(f"{cname} segment {i} (T={CODE_LENS[i]}, speed {SPEEDS[i]}): vs decode {e:.2e} (rng) {en:.2e} (noise), vs oracle {eo:.2e}")
        assert e <= 1e-5, f"segment {i}"
        assert en <= 1e-5, f"segment {i} (explicit noise)"
        assert eo <= 1e-4, f"segment {i} vs oracle"


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_no_leakage_across_segments(dtype):
    m, _, _ = _engine("small", dtype)
    outs = [_run(m, _six(swap2=swap), speeds=SPEEDS) for swap in (False, True)]
    for i in range(6):
        if i != 2:
            assert torch.equal(outs[0][i], outs[1][i]), f"segment {i} changed when segment 2 changed"
    assert not torch.equal(outs[0][2], outs[1][2])


def test_gap_rows_are_zero_in_the_post_layout():
    from gsv import _lib
    m, cfg, _ = _engine("small", torch.float32)
    _run(m, _six(), speeds=SPEEDS)
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
    cl, pl, sp = (C.c_int * n)(*CODE_LENS), (C.c_int * n)(*PHONE_LENS), (C.c_double * n)(*SPEEDS)

    def seg_map(level):
        rows = C.c_int64(0)
        _lib.check(_lib.lib().gsv_vits_segment_map_speed(C.byref(vc), n, cl, pl, sp, level, None, 0, C.byref(rows)))
        buf = (C.c_int32 * rows.value)()
        _lib.check(_lib.lib().gsv_vits_segment_map_speed(C.byref(vc), n, cl, pl, sp, level, buf, rows.value, C.byref(rows)))
        return np.frombuffer(buf, dtype=np.int32).copy()

    IC = mc["inter_channels"]
    G = _lib.lib().gsv_vits_segment_gap(C.byref(vc))
    sf = seg_map(0)
    assert len(sf) == sum(FRAMES) + (n - 1) * G and (sf < 0).sum() == (n - 1) * G
    z = m.debug_tensor("z", IC * len(sf)).cpu().numpy().reshape(IC, len(sf))
    assert np.all(z[:, sf < 0] == 0)
    assert np.all(np.abs(z[:, sf >= 0]).max(axis=0) > 0), "a segment row of z is all zero"
    last = vc.n_ups - 1
    sl = seg_map(last)
    ch = 2 * (mc["upsample_initial_channel"] >> vc.n_ups)
    g = m.debug_tensor("gen_last_in", ch * len(sl)).cpu().numpy().reshape(ch, len(sl))
    assert np.all(g[:, sl < 0] == 0)
    assert np.all(np.abs(g[:, sl >= 0]).max(axis=0) > 0), "a segment row of gen_last_in is all zero"


def test_fp16_against_fp32_isolated_decodes():
    """8 segments of T=100 on the full v2 config, speeds 1.25 / 0.9 / 1.0 in turn, explicit noise: the fp16 segmented
    pass against the fp32 engine's isolated decode at that speed, held to the bar of test_production_shape_fp16."""
    m16, cfg, _ = _engine("v2", torch.float16)
    m32, _, _ = _engine("v2", torch.float32)
    n, T = 8, 100
    speeds = [(1.25, 0.9, 1.0)[i % 3] for i in range(n)]
    frames = [2 * T if s == 1 else int(2 * T / s) + 1 for s in speeds]
    segs = []
    for i in range(n):
        codes, text = _seg_inputs(T, 20 + (i * 7) % 31, f"prod{i}")
        segs.append((codes, text, _voice(100 + i, tr=20 + i), 7000 + i))
    IC = cfg["model"]["inter_channels"]
    noise = [S.hash_normal(f"spd_prod_noise{i}", (IC, f), 9) for i, f in enumerate(frames)]
    out = _run(m16, segs, speeds=speeds, noise=noise)
    for i, (codes, text, v, seed) in enumerate(segs):
        ref = _alone(m32, codes, text, v, seed, speeds[i], noise=noise[i])
        assert out[i].shape == ref.shape
        err = out[i].float() - ref
        mx, rel = err.abs().max().item(), (err.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()
        print(f"fp16 segment {i} (speed {speeds[i]}): max-abs {mx:.3e}, relative rms {rel:.3e}")
        assert mx <= 2e-2, f"segment {i}"
        assert rel <= 0.03, f"segment {i}"


def test_errors_do_not_crash():
    from gsv import _lib
    m, _, _ = _engine("small", torch.float32)
    segs = _six()[2:4]
    good = _run(m, segs, speeds=[1.5, 1.0])
    with pytest.raises(ValueError):
        _run(m, segs, speeds=[1.5])
    with pytest.raises(ValueError):
        _run(m, segs, speeds=[1.5, 1.0, 1.0])
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            _run(m, segs, speeds=[1.5, bad])
    # the library's own checks, past the binding's
    l = _lib.lib()
    cd = torch.cat([s[0].reshape(-1) for s in segs]).to(torch.int32).contiguous()
    tx = torch.cat([s[1].reshape(-1) for s in segs]).to(torch.int32).contiguous()
    wav = torch.empty(4 * (12 + 74) * 16, device=DEV)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        rc = l.gsv_vits_decode_segments_speed(m._h, 2, cd.data_ptr(), (C.c_int * 2)(6, 37), tx.data_ptr(), (C.c_int * 2)(23, 40),
                                              (C.c_int * 2)(0, 1), (C.c_uint64 * 2)(0, 0), (C.c_double * 2)(1.5, bad), None, 0.5,
                                              wav.data_ptr(), None)
        assert rc != 0 and b"speed" in l.gsv_last_error()
    torch.cuda.synchronize()
    again = _run(m, segs, speeds=[1.5, 1.0])                   # the engine still decodes a valid call
    assert all(torch.equal(a, b) for a, b in zip(good, again))
    ref = _alone(m, *segs[0], 1.5)
    assert (again[0].float() - ref).abs().max().item() <= 1e-5
