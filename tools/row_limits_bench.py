"""Per-step device time of the AR decode's two call forms on this build: the scalar call, and the call that brings per-row
sampling values and limits (gsv_t2s_set_row_sampling / gsv_t2s_set_row_limits), equal to the scalars so that both decode the
same tokens.  The fp16 persistent engine on the v2 shape at B = 32 and B = 128, 100 steps: device time of the persistent launch
per step (gsv_t2s_decode_info), the two forms in alternating order, one JSON line per batch size with every run's time, the
medians and the min..max spread.

    python tools/row_limits_bench.py [--runs 1] [--steps 100]

A comparison of two commits runs this on both checkouts in separate processes, in alternating pairs (DESIGN.md sections 4t, 5).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gpt-sovits_amd")):
    sys.path.insert(0, p)

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=1, help="timed runs of each call form, after one warm-up run of each")
    ap.add_argument("--steps", type=int, default=100)
    a = ap.parse_args()
    from gsv import synthetic as S
    from gsv.AR.models.t2s_model import Text2SemanticDecoder
    dev = "cuda:0"
    cfg = S.T2S_V2_CONFIG
    sd = S.make_t2s_state_dict(cfg, seed=0, suppress_eos=True)
    eng = Text2SemanticDecoder(cfg, device=dev, dtype=torch.float16, max_batch=128, max_seq=80 + 100 + a.steps + 8)
    eng.load_state_dict(sd)
    for B in (32, 128):
        xs = [torch.from_numpy(S.hash_ints(f"rl_x{i}", 80, cfg["model"]["phoneme_vocab_size"], 0)).long().to(dev) for i in range(B)]
        pr = [torch.from_numpy(S.hash_ints(f"rl_p{i}", 100, 1024, 0)).long().to(dev) for i in range(B)]
        berts = [torch.zeros(1024, 80, device=dev) for _ in range(B)]
        ms = {False: [], True: []}

        def run(per_row):
            kw = dict(row_sampling=[(15, 1.0, 1.0, 1.35)] * B, row_limits=[(1, a.steps, a.steps + 1)] * B) if per_row else {}
            y, i = eng._run(xs, pr, berts, 15, 1.0, a.steps, 1.0, 1.35, eos_mask_steps=1, max_steps=a.steps + 1, seed=1, **kw)
            mode, dms, steps = eng.decode_info()
            assert mode == 1 and i == [a.steps] * B
            return [t.tolist() for t in y], dms / steps
        base, _ = run(False)
        assert run(True)[0] == base
        for k in range(a.runs):
            for per_row in ((False, True) if k % 2 == 0 else (True, False)):
                y, t = run(per_row)
                assert y == base
                ms[per_row].append(round(t, 4))
        print(json.dumps(dict(record="row_tables_step", B=B, steps=a.steps, runs=a.runs,
                              scalar_ms=round(statistics.median(ms[False]), 4), per_row_ms=round(statistics.median(ms[True]), 4),
                              scalar_spread=[min(ms[False]), max(ms[False])], per_row_spread=[min(ms[True]), max(ms[True])],
                              scalar_runs=ms[False], per_row_runs=ms[True])), flush=True)


if __name__ == "__main__":
    main()
