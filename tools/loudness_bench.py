"""Cost of loudness normalisation on the device: 32 fragments x 4 s of fp16 audio at 32 kHz, each with a
0.3 s gap per sentence.  Medians of 7 (after one warm-up call), device time between two events, in ms:

  (a) rate      gsv_postprocess_groups_rate, identity filter, int16: the path without loudness, the yardstick
  (b) fragment  gsv_postprocess_groups_loud, one span per fragment (its gaps included)
  (c) sentence  the same audio as 4 sentences per fragment, one span per sentence
  (d) mulaw     (b) with 32000 -> 8000 and mu-law output
  (e) host      the fp64 mirror on the host for context: the int16 of (a) copied back, scipy lfilter, blocks, gates, gain,
                wall time
  floor         (3 x source bytes + output bytes) / 6.3 TB/s: the meter reads the source twice, the write launch once

    python tools/loudness_bench.py [--fragments 32] [--seconds 4] [--out profiles/loudness_bench.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpt-sovits_amd"))

from gsv import _lib, audio_io  # noqa: E402

DEV = "cuda:0"
HBM = 6.3e12
RATE = 32000


def _device_ms(fn, reps=7):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def _host_meter(pcm, rate):
    """the definition of include/gsv.h in fp64 with scipy: -> the gain towards -20 LUFS"""
    from scipy.signal import lfilter
    k = audio_io.k_weighting(rate)
    y = lfilter(*k["highpass"], lfilter(*k["shelf"], pcm.astype(np.float64) / 32768.0))
    s = k["sub_block"]
    J = y.shape[0] // s
    e = (y[:J * s] ** 2).reshape(J, s).sum(axis=1)
    z = (e[:-3] + e[1:-2] + e[2:-1] + e[3:]) / (4.0 * s)
    lv = -0.691 + 10.0 * np.log10(np.maximum(z, 1e-300))
    keep = lv > -70.0
    keep &= lv > -0.691 + 10.0 * np.log10(z[keep].mean()) - 10.0
    return 10.0 ** ((-20.0 - (-0.691 + 10.0 * np.log10(z[keep].mean()))) / 20.0)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fragments", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.init(0)
    l = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n, length, gap = a.fragments, int(a.seconds * RATE), int(0.3 * RATE)
    g = torch.Generator().manual_seed(1)
    wav = ((torch.rand(n * length + 1, generator=g) * 1.8 - 0.9) * 0.2).to(DEV, torch.float16)
    lines = []

    def case(per, sr_out, enc, spans_of):
        """`per` sentences per fragment; spans_of(first sentence of the fragment) -> its spans, or None for the rate call"""
        m = n * per
        frags = list(torch.split(wav[1:], length // per))[:m]           # views at an odd element offset
        lens = (C.c_int * m)(*[length // per] * m)
        ptrs = (C.c_void_p * m)(*[f.data_ptr() for f in frags])
        gn, gg = (C.c_int * n)(*[per] * n), (C.c_int * n)(*[gap] * n)
        off = (C.c_longlong * (n + 1))()
        spans = [] if spans_of is None else [s for i in range(n) for s in spans_of(i * per)]
        arr = (_lib.LoudSpan * max(len(spans), 1))(*spans)
        need = int(l.gsv_postprocess_groups_loud_workspace(lens, m, gn, gg, n, RATE, len(spans)))
        table = torch.empty(need, dtype=torch.uint8).pin_memory()
        work = torch.empty(need, dtype=torch.uint8, device=DEV)
        report = torch.empty(16 * max(len(spans), 1), dtype=torch.uint8, device=DEV)
        hd, up, down = audio_io.output_filter_device(RATE, sr_out, torch.device(DEV))
        fmt = audio_io.ENCODINGS[enc]
        total = n * audio_io.resampled_len(per * (length // per + gap), RATE, sr_out)
        out = torch.empty(total, dtype=torch.int16 if fmt == 0 else torch.uint8, device=DEV)

        def call():
            if spans_of is None:
                _lib.check(l.gsv_postprocess_groups_rate(ptrs, lens, m, _lib.GSV_F16, gn, gg, n, out.data_ptr(), off, table.data_ptr(),
                                                         work.data_ptr(), hd.data_ptr(), int(hd.numel()), up, down, fmt, st), "rate")
            else:
                _lib.check(l.gsv_postprocess_groups_loud(ptrs, lens, m, _lib.GSV_F16, gn, gg, n, out.data_ptr(), off, table.data_ptr(),
                                                         work.data_ptr(), hd.data_ptr(), int(hd.numel()), up, down, fmt, RATE, arr,
                                                         len(spans), report.data_ptr(), st), "loud")
        ms = _device_ms(call)
        floor = ((1 if spans_of is None else 3) * m * (length // per) * 2 + out.numel() * out.element_size()) / HBM * 1e3
        return ms, floor, out, (frags, table, work, report)

    t_a, f_a, pcm, _ = case(1, RATE, "pcm_s16", None)
    t_b, f_b, _, _ = case(1, RATE, "pcm_s16", lambda f: [_lib.LoudSpan(f, 1, 1, -20.0, 0.0)])
    t_c, f_c, _, _ = case(4, RATE, "pcm_s16", lambda f: [_lib.LoudSpan(f + i, 1, 0, -20.0, 0.0) for i in range(4)])
    t_d, f_d, _, _ = case(1, 8000, "mulaw", lambda f: [_lib.LoudSpan(f, 1, 1, -20.0, 0.0)])

    def host():
        h = pcm.cpu().numpy().reshape(n, length + gap)
        for i in range(n):
            np.clip(np.trunc(h[i] * _host_meter(h[i], RATE)), -32768, 32767).astype(np.int16)
    host()
    times = []
    for _ in range(7):
        t = time.perf_counter()
        host()
        times.append((time.perf_counter() - t) * 1e3)
    t_e = statistics.median(times)
    lines.append(f"{n} fragments x {a.seconds:g} s, fp16, {RATE} Hz; medians of 7, ms")
    lines.append(f"(a) rate, identity, int16          {t_a:8.3f}   floor {f_a:.4f}")
    lines.append(f"(b) loud, fragment scope           {t_b:8.3f}   floor {f_b:.4f}   (b)/(a) = {t_b / t_a:.2f}")
    lines.append(f"(c) loud, sentence scope, 4 each   {t_c:8.3f}   floor {f_c:.4f}")
    lines.append(f"(d) loud, 32000 -> 8000 mu-law     {t_d:8.3f}   floor {f_d:.4f}")
    lines.append(f"(e) host fp64 mirror with copy     {t_e:8.2f}")
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
