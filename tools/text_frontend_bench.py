#!/usr/bin/env python3
"""zh text front-end: the per-sentence BERT loop (`BertFeature.__call__` once per sentence, what `TextPreprocessor.preprocess`
does; unchanged by the packed pass, hence the parent commit's cost) against one `BertFeature.batch` call over the same
sentences, in the same process, alternating.  Full-size synthetic BERT (22 of 24 BERT-large layers, test vocabulary);
sentence counts 1 / 8 / 32 / 140 at 12 / 30 / 60 characters; then a sweep of `max_tokens` on the largest job.  Times are host
wall clock around work that ends in a stream synchronise (both paths end in a device-to-host copy), medians of --reps runs
after --warmup runs (measurement tool, not product code; not part of bench.py).

    python tools/text_frontend_bench.py > profiles/text_frontend.json         # prints one JSON line
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpt-sovits_amd"))
import torch  # noqa: E402

from gsv import synthetic as S  # noqa: E402
from gsv.feature_extractor.bert import BertFeature  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--counts", type=int, nargs="*", default=[1, 8, 32, 140])
ap.add_argument("--chars", type=int, nargs="*", default=[12, 30, 60])
ap.add_argument("--sweep", type=int, nargs="*", default=[512, 1024, 2048, 4096, 8192, 16384])
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("text_frontend_bench needs the MI355X: there is no CPU path to time")

ZH = [c for c in S.BERT_TEST_VOCAB[5:] if not c.isascii()]
bf = BertFeature(device="cuda:0", state_dict=S.make_bert_state_dict(seed=0, layers=22), vocab=S.BERT_TEST_VOCAB)


def sentences(n, chars):
    return ["".join(ZH[(i * 7 + k * 13 + i // 5) % len(ZH)] for i in range(chars)) for k in range(n)]


def loop(texts):
    return [bf(t).float().cpu() for t in texts]                  # TextPreprocessor.get_bert_feature


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median_pair(a, b):
    """medians (ms) of a and b, run alternately"""
    for _ in range(args.warmup):
        a(); b()
    ta, tb = [], []
    for _ in range(args.reps):
        ta.append(timed(a)); tb.append(timed(b))
    return statistics.median(ta), statistics.median(tb), max(ta) - min(ta), max(tb) - min(tb)


rows = []
for chars in args.chars:
    for n in args.counts:
        texts = sentences(n, chars)
        p0 = bf.passes
        out = bf.batch(texts)
        passes = bf.passes - p0
        ref = loop(texts)
        diff = max(float((o - r).abs().max()) for o, r in zip(out, ref))
        tl, tb, sl, sb = median_pair(lambda: loop(texts), lambda: bf.batch(texts))
        rows.append({"sentences": n, "chars": chars, "tokens": n * (chars + 2), "passes": passes, "loop_ms": round(tl, 3),
                     "batch_ms": round(tb, 3), "loop_spread_ms": round(sl, 3), "batch_spread_ms": round(sb, 3),
                     "speedup": round(tl / tb, 2), "max_abs_batch_vs_loop": round(diff, 5)})
sweep = []
texts = sentences(max(args.counts), max(args.chars))
for mt in args.sweep:
    p0 = bf.passes
    bf.batch(texts, max_tokens=mt)
    passes = bf.passes - p0
    ta, tb, _, sb = median_pair(lambda: bf.batch(texts, max_tokens=mt), lambda: bf.batch(texts, max_tokens=mt))
    sweep.append({"max_tokens": mt, "passes": passes, "batch_ms": round(min(ta, tb), 3), "spread_ms": round(sb, 3)})
print(json.dumps({"tool": "text_frontend_bench", "device": torch.cuda.get_device_name(0), "layers": bf.layers_used,
                  "default_max_tokens": bf.MAX_TOKENS, "reps": args.reps, "rows": rows,
                  "sweep": {"sentences": len(texts), "chars": max(args.chars), "tokens": sum(len(t) + 2 for t in texts),
                            "points": sweep}}))
