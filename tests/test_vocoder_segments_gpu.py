"""GPU: gsv_vocoder_forward_segments (`BigVGAN.forward_segments`, the v4 `Generator.forward_segments`) -- several mels through
one pass of the generator, each segment as `forward` of that segment alone gives it.

Bars: fp32 within 1e-5 of the segment's own forward (the bar of the segmented SoVITS decode) and 2e-4 of oracle/vocoder_oracle.py
(the fp32 vocoder bar of tests/test_vits_gpu.py); fp16 within 3e-2 max-abs and 5 % relative rms (the fp16 vocoder bar there)."""
import ctypes as C
import functools
import math

import pytest
import torch

from gsv import _lib, synthetic as S
from oracle import cases, vocoder_oracle
from test_vits_gpu import _vocoder

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FRAMES = [1, 2, 7, 16, 17, 40]
FULL = {"bigvgan": ("voc_bigvgan_v2", [60, 33, 7]), "hifigan": ("voc_hifigan_v4", [50, 21, 3])}


def _mels(frames, tag):
    return [S.hash_symmetric(f"vseg_mel_{tag}{i}", (1, 100, f), 2.0, 7) for i, f in enumerate(frames)]


@functools.lru_cache(maxsize=None)
def _small(kind):
    """config, weights, the six mels and the oracle's waveform of each alone; computed once"""
    cfg = S.small_vocoder_config(kind)
    sd = S.make_vocoder_state_dict(cfg, seed=11)
    mels = _mels(FRAMES, kind)
    ref = [getattr(vocoder_oracle, kind)(sd, cfg, m) for m in mels]
    return cfg, sd, mels, ref


@functools.lru_cache(maxsize=None)
def _engine(kind, dtype):
    cfg, sd, _, _ = _small(kind)
    return _vocoder(cfg, sd, dtype)


def _errs(a, b):
    a, b = a.float().cpu().double(), b.float().cpu().double()
    return float((a - b).abs().max()), float((a - b).pow(2).mean().sqrt() / max(float(b.pow(2).mean().sqrt()), 1e-12))


@pytest.mark.parametrize("kind", ["bigvgan", "hifigan"])
def test_small_fp32_each_segment_equals_its_own_forward_and_the_oracle(kind):
    cfg, _, mels, ref = _small(kind)
    m = _engine(kind, torch.float32)
    up = math.prod(cfg["upsample_rates"])
    out = m.forward_segments([x.to(DEV) for x in mels])
    assert len(out) == len(mels)
    for s, (x, w, r) in enumerate(zip(mels, out, ref)):
        assert w.shape == (1, 1, x.shape[2] * up) == r.shape
        own = m(x.to(DEV))
        d_own, d_ref = _errs(w, own)[0], _errs(w, r)[0]
        print(f"{kind} fp32 segment {s} ({x.shape[2]} frames): vs own forward {d_own:.3e}, vs oracle {d_ref:.3e}")
        assert d_own <= 1e-5 and d_ref <= 2e-4
        assert float(w.abs().max()) > 0


@pytest.mark.parametrize("kind", ["bigvgan", "hifigan"])
def test_neighbours_do_not_matter(kind):
    """the same segments in reversed order: every segment keeps its samples"""
    _, _, mels, _ = _small(kind)
    m = _engine(kind, torch.float32)
    fwd = m.forward_segments([x.to(DEV) for x in mels])
    rev = m.forward_segments([x.to(DEV) for x in reversed(mels)])[::-1]
    for s, (a, b) in enumerate(zip(fwd, rev)):
        d = _errs(a, b)[0]
        print(f"{kind} segment {s}: forward order vs reversed order {d:.3e}")
        assert a.shape == b.shape and d <= 1e-5


@pytest.mark.parametrize("kind", ["bigvgan", "hifigan"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_one_segment_is_forward_itself(kind, dtype):
    _, _, mels, _ = _small(kind)
    m = _engine(kind, dtype)
    for x in (mels[0], mels[4]):
        one = m.forward_segments([x.to(DEV)])
        assert len(one) == 1 and torch.equal(one[0], m(x.to(DEV)))


@pytest.mark.parametrize("kind", ["bigvgan", "hifigan"])
def test_small_fp16_against_the_fp32_oracle(kind):
    _, _, mels, ref = _small(kind)
    out = _engine(kind, torch.float16).forward_segments([x.to(DEV) for x in mels])
    for s, (w, r) in enumerate(zip(out, ref)):
        mx, rel = _errs(w, r)
        print(f"{kind} fp16 segment {s} ({mels[s].shape[2]} frames): max-abs {mx:.3e}, relative rms {rel:.3e}")
        assert w.shape == r.shape and mx <= 3e-2 and rel <= 5e-2


@pytest.mark.parametrize("kind", ["bigvgan", "hifigan"])
def test_full_config_fp16_against_its_own_forward(kind):
    """BigVGAN-v2 24 kHz at 60 / 33 / 7 frames and the v4 HiFi-GAN at 50 / 21 / 3: the masked fused pairs and the wide conv
    routes the small config does not reach.  Each segment against the engine's own fp16 forward of it (no host oracle at
    full size).  The errors are printed; DESIGN.md section 4h records them once a run has been made."""
    name, frames = FULL[kind]
    cfg, sd, _ = cases.voc_case_inputs(cases.VOC_CASES[name])
    m = _vocoder(cfg, sd, torch.float16)
    mels = _mels(frames, "full_" + kind)
    up = math.prod(cfg["upsample_rates"])
    out = m.forward_segments([x.to(DEV) for x in mels])
    for s, (x, w) in enumerate(zip(mels, out)):
        own = m(x.to(DEV))
        mx, rel = _errs(w, own)
        print(f"{kind} full fp16 segment {s} ({x.shape[2]} frames): vs own forward max-abs {mx:.3e}, relative rms {rel:.3e}")
        assert w.shape == (1, 1, x.shape[2] * up) == own.shape
        assert mx <= 3e-2 and rel <= 5e-2


def test_bad_arguments_are_errors_and_the_handle_still_works():
    _, _, mels, _ = _small("bigvgan")
    m = _engine("bigvgan", torch.float32)
    e, l = m._e, _lib.lib()
    mel = torch.cat([x[0] for x in mels[:2]], 1).to(DEV).contiguous()
    wav = torch.zeros(3 * 16, device=DEV)
    st = C.c_void_p(e.stream.cuda_stream)
    ok = (C.c_int * 2)(1, 2)
    assert l.gsv_vocoder_forward_segments(e._h, None, 2, ok, wav.data_ptr(), st) != 0
    assert l.gsv_vocoder_forward_segments(e._h, mel.data_ptr(), 2, None, wav.data_ptr(), st) != 0
    assert l.gsv_vocoder_forward_segments(e._h, mel.data_ptr(), 2, ok, None, st) != 0
    assert l.gsv_vocoder_forward_segments(None, mel.data_ptr(), 2, ok, wav.data_ptr(), st) != 0
    assert l.gsv_vocoder_forward_segments(e._h, mel.data_ptr(), 0, ok, wav.data_ptr(), st) != 0
    assert l.gsv_vocoder_forward_segments(e._h, mel.data_ptr(), 4097, (C.c_int * 4097)(*([1] * 4097)), wav.data_ptr(), st) != 0
    assert l.gsv_vocoder_forward_segments(e._h, mel.data_ptr(), 2, (C.c_int * 2)(1, 0), wav.data_ptr(), st) != 0
    assert l.gsv_vocoder_forward_segments(e._h, mel.data_ptr(), 2, (C.c_int * 2)(1 << 19, 1 << 19), wav.data_ptr(), st) != 0
    assert b"2^24" in l.gsv_last_error()
    e.stream.synchronize()
    assert float(wav.abs().max()) == 0.0, "nothing was launched"
    with pytest.raises(ValueError):
        m.forward_segments([])
    with pytest.raises(ValueError):
        m.forward_segments([torch.zeros(1, 99, 4, device=DEV)])
    out = m.forward_segments([x.to(DEV) for x in mels[:2]])
    assert all(_errs(w, m(x.to(DEV)))[0] <= 1e-5 for w, x in zip(out, mels))
