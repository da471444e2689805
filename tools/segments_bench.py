"""Segmented SoVITS decode at the production shape: N segments x T codes, N distinct voices, fp16 synthetic v2 weights.
Prints one JSON line: wall, device and generator time of one SynthesizerTrn.decode_segments (median and range over the
iterations) and whether the masked fused ResBlock pairs ran.  A/B: run it again with GSV_NO_SEG_PAIR=1 in a separate
process (the switch is read once).  --speed S decodes every segment at speed S (decode_segments(speeds=...)) and also
times, in the same process, what the pipeline does without the shared pass: one decode(speed=S) per segment with its voice.

    python tools/segments_bench.py [--segments 32] [--codes 100] [--iters 10] [--fold] [--speed 1.25]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gpt-sovits_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, default=32)
    ap.add_argument("--codes", type=int, default=100)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--fold", action="store_true", help="also time the single-voice fold of the same codes (unmasked pairs)")
    ap.add_argument("--speed", type=float, default=1.0, help="speed of every segment; != 1 also times the per-segment decode loop")
    a = ap.parse_args()
    from gsv import _lib, synthetic as S
    from gsv.module.models import SynthesizerTrn
    dev = "cuda:0"
    cfg = S.VITS_V2_CONFIG
    d = cfg["data"]
    m = SynthesizerTrn(d["filter_length"] // 2 + 1, cfg["train"]["segment_size"] // d["hop_length"], n_speakers=d["n_speakers"],
                       version="v2", device=dev, dtype=torch.float16, n_symbols=cfg.get("n_symbols"), **cfg["model"])
    m.load_state_dict(S.make_vits_state_dict(cfg, seed=0))
    n, T = a.segments, a.codes
    codes = [torch.from_numpy(S.hash_ints(f"sb_codes{i}", T, 1024, 5)).view(1, 1, -1).to(dev) for i in range(n)]
    text = [torch.from_numpy(S.hash_ints(f"sb_text{i}", 20 + (i * 7) % 31, 732, 5)).view(1, -1).to(dev) for i in range(n)]
    voices = [([S.make_refer_spec(frames=150 + 7 * i, seed=100 + i).to(dev)], None) for i in range(n)]
    seeds = list(range(n))
    speed_kw = {} if a.speed == 1.0 else dict(speeds=[a.speed] * n)
    wall, devms, genms = [], [], []
    for it in range(a.iters + 2):                      # two warm-up passes (workspaces, voice slots)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.decode_segments(codes, text, voices, seeds, **speed_kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if it >= 2:
            dv, gn = m.last_timing()
            wall.append(dt * 1e3), devms.append(dv), genms.append(gn)
    route = int(_lib.lib().gsv_debug_last_pair_route(0)) & 0xFFFFFFFFFFFFFFFF
    med = statistics.median
    fold = {}
    if a.fold:
        fd = []
        for it in range(a.iters + 2):
            m.decode(torch.cat(codes, dim=-1), torch.cat(text, dim=-1), voices[0][0], seed=1)
            if it >= 2:
                fd.append(m.last_timing()[0])
        fold = {"fold_device_ms": [round(med(fd), 2), round(min(fd), 2), round(max(fd), 2)]}
    if a.speed != 1.0:
        lp = []
        for it in range(a.iters + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for c, t, v, sd in zip(codes, text, voices, seeds):
                m.decode(c, t, v[0], speed=a.speed, seed=sd)
            torch.cuda.synchronize()
            if it >= 2:
                lp.append((time.perf_counter() - t0) * 1e3)
        fold.update(speed=a.speed, loop_wall_ms=[round(med(lp), 2), round(min(lp), 2), round(max(lp), 2)])
    print(json.dumps({**fold, "segments": n, "codes": T, "audio_s": n * T / 25.0, "masked_pairs": bool((route >> 56) & 16),
                      "fused_pairs": (route & 255) == 8,
                      "wall_ms": [round(med(wall), 2), round(min(wall), 2), round(max(wall), 2)],
                      "device_ms": [round(med(devms), 2), round(min(devms), 2), round(max(devms), 2)],
                      "generator_ms": [round(med(genms), 2), round(min(genms), 2), round(max(genms), 2)]}))


if __name__ == "__main__":
    main()
