"""Per-step cost of the decode with per-row limits against without (gsv_t2s_set_row_limits): the fp16 persistent engine on
the v2 shape at B = 32 and B = 128, 100 steps, the limits equal to the call's scalars so that both decode the same tokens.
Device time of the persistent launch per step (gsv_t2s_decode_info), alternating pairs, medians and the min..max spread.

    python tools/row_limits_bench.py [--pairs 7] [--steps 100]
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
    ap.add_argument("--pairs", type=int, default=7)
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

        def run(limits):
            kw = dict(row_limits=[(1, a.steps, a.steps + 1)] * B) if limits else {}
            y, i = eng._run(xs, pr, berts, 15, 1.0, a.steps, 1.0, 1.35, eos_mask_steps=1, max_steps=a.steps + 1, seed=1, **kw)
            mode, dms, steps = eng.decode_info()
            assert mode == 1 and i == [a.steps] * B
            return [t.tolist() for t in y], dms / steps
        base, _ = run(False)
        for k in range(a.pairs):
            for limits in ((False, True) if k % 2 == 0 else (True, False)):
                y, t = run(limits)
                assert y == base
                ms[limits].append(t)
        print(json.dumps(dict(record="row_limits_step", B=B, steps=a.steps, pairs=a.pairs,
                              off_ms=round(statistics.median(ms[False]), 4), on_ms=round(statistics.median(ms[True]), 4),
                              off_spread=[round(min(ms[False]), 4), round(max(ms[False]), 4)],
                              on_spread=[round(min(ms[True]), 4), round(max(ms[True]), 4)])), flush=True)


if __name__ == "__main__":
    main()
