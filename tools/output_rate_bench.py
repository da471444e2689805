"""Cost of an output sample rate / encoding on the device: 32 fragments x 4 s of fp16 audio, each one
sentence with a 0.3 s gap, for 32000 -> 8000 (mu-law), 32000 -> 16000, 32000 -> 44100 and 24000 -> 48000 (int16).

Per pair, medians of 7 (after one warm-up call), in ms:
  fused        one gsv_postprocess_groups_rate call (peaks + resample/convert), device time between two events
  composed     the existing pieces per fragment: gsv_postprocess_f32, audio_io.resample_segments, a torch conversion to int16
               (x 32768, clamp, truncate; mu-law is not composed: torch has no G.711, so its row is the int16 composition)
  host         audio_io.resample (scipy, fp64) on the default int16 result of every fragment, wall time
  default      gsv_postprocess_groups on the same fragments at the model's rate, for scale
  floor        (input bytes + output bytes) / 6.3 TB/s

    python tools/output_rate_bench.py [--fragments 32] [--seconds 4] [--json out.json]
"""
import argparse
import ctypes as C
import json
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
CASES = [(32000, 8000, "mulaw"), (32000, 16000, "pcm_s16"), (32000, 44100, "pcm_s16"), (24000, 48000, "pcm_s16")]
HBM = 6.3e12


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


def _wall_ms(fn, reps=7):
    fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--fragments", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    _lib.init(0)
    l = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = []
    for sr_in, sr_out, enc in CASES:
        n, length, gap = a.fragments, int(a.seconds * sr_in), int(0.3 * sr_in)
        g = torch.Generator().manual_seed(1)
        wav = (torch.rand(n * length + 1, generator=g) * 1.8 - 0.9).to(DEV, torch.float16)
        frags = list(torch.split(wav[1:], length))                       # views at an odd element offset, as torch.split hands them
        lens = (C.c_int * n)(*[length] * n)
        ptrs = (C.c_void_p * n)(*[f.data_ptr() for f in frags])
        gn, gg = (C.c_int * n)(*[1] * n), (C.c_int * n)(*[gap] * n)
        off = (C.c_longlong * (n + 1))()
        need = max(int(l.gsv_postprocess_groups_rate_workspace(lens, n, n)), int(l.gsv_postprocess_groups_workspace(lens, n)))
        table = torch.empty(need, dtype=torch.uint8).pin_memory()
        work = torch.empty(need, dtype=torch.uint8, device=DEV)
        hd, up, down = audio_io.output_filter_device(sr_in, sr_out, torch.device(DEV))
        fmt = audio_io.ENCODINGS[enc]
        m = audio_io.resampled_len(length + gap, sr_in, sr_out)
        out = torch.empty(n * m, dtype=torch.int16 if fmt == 0 else torch.uint8, device=DEV)

        def fused():
            _lib.check(l.gsv_postprocess_groups_rate(ptrs, lens, n, _lib.GSV_F16, gn, gg, n, out.data_ptr(), off, table.data_ptr(),
                                                     work.data_ptr(), hd.data_ptr(), int(hd.numel()), up, down, fmt, st), "rate")
        f32 = torch.empty(n * (length + gap), dtype=torch.float32, device=DEV)
        one_n, one_p = [(C.c_int * 1)(length) for _ in range(n)], [(C.c_void_p * 1)(f.data_ptr()) for f in frags]

        def composed():
            for i in range(n):
                seg = f32[i * (length + gap):(i + 1) * (length + gap)]
                _lib.check(l.gsv_postprocess_f32(one_p[i], one_n[i], 1, _lib.GSV_F16, gap, seg.data_ptr(), st), "f32")
                y, _, _ = audio_io.resample_segments(seg, [0], [length + gap], sr_in, sr_out)
                (y * 32768.0).clamp_(-32768.0, 32767.0).trunc_().to(torch.int16)
        pcm = torch.empty(n * (length + gap), dtype=torch.int16, device=DEV)

        def default():
            _lib.check(l.gsv_postprocess_groups(ptrs, lens, n, _lib.GSV_F16, gn, gg, n, pcm.data_ptr(), off, table.data_ptr(),
                                                work.data_ptr(), st), "groups")
        t_fused, t_comp, t_def = _device_ms(fused), _device_ms(composed), _device_ms(default)
        host_pcm = pcm.cpu().numpy().reshape(n, length + gap)

        def host():
            for i in range(n):
                y = audio_io.resample(host_pcm[i].astype(np.float32) / 32768.0, sr_in, sr_out)
                np.clip(np.trunc(y * 32768.0), -32768, 32767).astype(np.int16)
        t_host = _wall_ms(host)
        floor = (n * length * 2 + out.numel() * out.element_size()) / HBM * 1e3
        rows.append(dict(sr_in=sr_in, sr_out=sr_out, encoding=enc, fragments=n, seconds=a.seconds, taps=int(hd.numel()), up=up, down=down,
                         fused_ms=t_fused, composed_ms=t_comp, host_ms=t_host, default_ms=t_def, floor_ms=floor))
        print(f"{sr_in} -> {sr_out} {enc:8s} fused {t_fused:8.3f} ms  composed {t_comp:8.3f} ms  host {t_host:9.2f} ms  "
              f"default {t_def:7.3f} ms  floor {floor:.4f} ms", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
