"""GPU: spectrogram_torch_segments (one gsv_op_frame_seg, one DFT GEMM at M = sum T_s, a magnitude per audio; DESIGN.md section
4m) on four audios of 0.1 .. 0.5 s at 32 kHz against an fp64 numpy mirror (reflect padding, periodic Hann, np.fft.rfft,
sqrt(re^2 + im^2 + 1e-8)).

The bars: spectrogram_torch's own error against that mirror on the same audios (relative rms and max abs, the worst audio of
each), times two -- the project's precedent in test_hubert_batch_gpu.py: the GEMM's route may differ with M, its arithmetic
does not get worse than the per-audio call's by more than that."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_FFT, HOP, WIN, SR = 2048, 640, 2048, 32000
LENS = [3200, 7777, 12001, 16000]


def _mirror(x):
    pad = (N_FFT - HOP) // 2
    xp = np.pad(x.astype(np.float64), (pad, pad), mode="reflect")
    T = (xp.shape[0] - N_FFT) // HOP + 1
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(WIN) / WIN)             # periodic Hann
    fr = np.stack([xp[t * HOP:t * HOP + N_FFT] * w for t in range(T)])
    f = np.fft.rfft(fr, axis=1)
    return np.sqrt(f.real ** 2 + f.imag ** 2 + 1e-8).T                     # [bins][T]


def _errs(got, ref):
    d = got.astype(np.float64) - ref
    return float(np.sqrt((d ** 2).sum() / (ref ** 2).sum())), float(np.abs(d).max())


@functools.lru_cache(maxsize=None)
def _data():
    from gsv import synthetic as S
    from gsv.module.mel_processing import spectrogram_torch, spectrogram_torch_segments
    xs = [S.make_waveform(n, 300 + k, sr=SR) for k, n in enumerate(LENS)]
    refs = [_mirror(x.numpy()) for x in xs]
    single = [spectrogram_torch(x.unsqueeze(0).to(DEV), N_FFT, SR, HOP, WIN) for x in xs]
    starts, a = [], 11
    for n in LENS:
        starts.append(a)
        a += n + 5
    stream = torch.full((a,), 9.0)
    for x, o in zip(xs, starts):
        stream[o:o + x.numel()] = x
    packed = spectrogram_torch_segments(stream.to(DEV), starts, LENS, N_FFT, SR, HOP, WIN)
    torch.cuda.synchronize()
    return xs, refs, single, packed, stream, starts


def test_shapes_and_order():
    xs, refs, single, packed, _, _ = _data()
    assert len(packed) == len(LENS)
    for ref, one, pk in zip(refs, single, packed):
        assert pk.dtype == torch.float32 and pk.shape == one.shape == (1, N_FFT // 2 + 1, ref.shape[1])
    assert len({r.shape[1] for r in refs}) == len(LENS)                    # four different frame counts: a swap would show


def test_within_twice_the_per_audio_call_s_error():
    xs, refs, single, packed, _, _ = _data()
    one = [_errs(s[0].cpu().numpy(), r) for s, r in zip(single, refs)]
    pk = [_errs(p[0].cpu().numpy(), r) for p, r in zip(packed, refs)]
    bar_rms, bar_abs = 2 * max(e[0] for e in one), 2 * max(e[1] for e in one)
    print("spectrogram_torch          rel rms / max abs per audio:", [(f"{a:.3e}", f"{b:.3e}") for a, b in one])
    print("spectrogram_torch_segments rel rms / max abs per audio:", [(f"{a:.3e}", f"{b:.3e}") for a, b in pk])
    assert bar_rms < 1e-4                                                   # the per-audio call itself is an fp32 DFT
    for a, b in pk:
        assert a <= bar_rms and b <= bar_abs


def test_short_audio_is_refused_before_any_launch():
    from gsv.module.mel_processing import spectrogram_torch_segments
    _, _, _, _, stream, starts = _data()
    with pytest.raises(ValueError, match="shorter than the reflect padding"):
        spectrogram_torch_segments(stream.to(DEV), [starts[0], starts[1]], [LENS[0], 704], N_FFT, SR, HOP, WIN)
