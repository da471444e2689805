#!/usr/bin/env python3
"""AR decode sessions (continuous batching) against static launches under unequal output lengths (measurement tool, not
product code).

fp16, the full-size synthetic v2 decoder, a queue of 256 rows of the benchmark's configs[1] shape (80 phonemes, 100 prompt
tokens).  The synthetic weights never emit EOS, so every row's length is imposed, in both modes the same way, through the
teacher-forcing hook (gsv_t2s_set_debug's force_tokens): row i is forced hash tokens for L_i steps and EOS at step L_i, with
L_i from a fixed hash distribution over 50 .. 350.  The sampling kernel still runs at every step; only the token taken differs.

In one process:
  static    launches of 32 / 128 consecutive rows through Text2SemanticDecoder._run, as TTS._ar_stage cuts a group today
            (plan_batch sorts by input length, which is equal here, so the queue order stands); a launch lasts as long as its
            longest row;
  session   one T2SSession of 32 / 64 / 128 slots over the whole queue, chunk in {8, 16, 32, 64} steps per advance and
            admit_min in {1, slots/8, slots/4, slots/2} free slots per admission.
Medians of 7 runs (--reps).  Per line: wall ms for the queue, generated tokens per second, slot occupancy (live row-steps /
slot-steps), and for sessions the median admission time by row count, the adopt launch against its byte floor at 6.3 TB/s
(bytes read + bytes written), and the relaunch overhead per advance = wall time of advance(k) minus k times the in-launch
step time (gsv_t2s_decode_info device ms / steps of the static launch at that batch size).

    python tools/continuous_ar_bench.py > profiles/continuous_ar.txt
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpt-sovits_amd"))
import torch  # noqa: E402

from gsv import synthetic as S  # noqa: E402
from gsv.AR.models.t2s_model import Text2SemanticDecoder, admit_count  # noqa: E402

DEV = "cuda:0"
N, X, P, LO, HI = 256, 80, 100, 50, 350
HBM = 6.3e12


def med(v):
    return statistics.median(v) if v else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", type=int, default=N)
    ap.add_argument("--slots", type=int, nargs="*", default=[32, 64, 128])
    ap.add_argument("--chunks", type=int, nargs="*", default=[8, 16, 32, 64])
    a = ap.parse_args()
    n = a.rows
    cfg = S.T2S_V2_CONFIG
    m = cfg["model"]
    V, EOS = m["vocab_size"], m["vocab_size"] - 1
    eng = Text2SemanticDecoder(cfg, device=DEV, dtype=torch.float16, max_batch=128, max_seq=X + P + 2 + HI + 1 + 27)
    eng.load_state_dict(S.make_t2s_state_dict(cfg, seed=0, suppress_eos=True))
    xs = [torch.from_numpy(S.hash_ints(f"ca_x{i}", X, m["phoneme_vocab_size"], 0)).long().to(DEV) for i in range(n)]
    berts = [torch.zeros(1024, X) for _ in range(n)]
    prompts = [torch.from_numpy(S.hash_ints(f"ca_p{i}", P, EOS, 0)).long().to(DEV) for i in range(n)]
    lens = (S.hash_ints("ca_len", n, HI - LO + 1, 0) + LO).tolist()
    force = torch.from_numpy(S.hash_ints("ca_tok", n * (HI + 1), EOS, 0)).to(torch.int32).reshape(n, HI + 1)
    for i, L in enumerate(lens):
        force[i, L:] = EOS
    force = force.to(DEV)
    keys = [(0, i) for i in range(n)]
    kw = dict(top_k=15, top_p=1.0, temperature=1.0, repetition_penalty=1.35, early_stop_num=HI)
    tokens = sum(lens)
    print(f"# AR decode sessions vs static launches: MI355X, fp16 v2 decoder, {n} rows of {X} phonemes + {P} prompt tokens, lengths "
          f"hash-uniform {LO}..{HI} (min {min(lens)}, median {med(lens):.0f}, max {max(lens)}, sum {tokens}), EOS teacher-forced; "
          f"medians of {a.reps}")

    def sync():
        torch.cuda.synchronize()

    # ---- static launches ----
    step_ms = {}
    print("# static: launches of B consecutive rows (Text2SemanticDecoder._run)")
    print(f"{'mode':>8} {'B':>4} {'chunk':>5} {'admit_min':>9} {'ms':>9} {'tok/s':>9} {'occupancy':>9}")
    for B in (32, 128):
        times, per_step = [], []
        slot_steps = sum(B * max(lens[lo:lo + B]) for lo in range(0, n, B))
        for rep in range(a.reps + 1):
            sync()
            t0 = time.perf_counter()
            for lo in range(0, n, B):
                hi = min(lo + B, n)
                y, idx = eng._run(xs[lo:hi], prompts[lo:hi], berts[lo:hi], kw["top_k"], kw["top_p"], kw["early_stop_num"],
                                  kw["temperature"], kw["repetition_penalty"], eos_mask_steps=1, force_tokens=force[lo:hi],
                                  rng_keys=keys[lo:hi])
                assert idx == lens[lo:hi], "the forced lengths must be the decoded lengths"
                mode, dms, _ = eng.decode_info()
                assert mode == 1, "the persistent engine must run"
                per_step.append(dms / max(lens[lo:hi]))
            sync()
            if rep:                           # the first run is the warm-up
                times.append((time.perf_counter() - t0) * 1e3)
        step_ms[B] = med(per_step)
        print(f"{'static':>8} {B:>4} {'-':>5} {'-':>9} {med(times):>9.1f} {tokens / med(times) * 1e3:>9.0f} {tokens / slot_steps:>9.3f}"
              f"   in-launch step {step_ms[B] * 1e3:.0f} us", flush=True)
    step_ms[64] = (step_ms[32] + step_ms[128]) / 2   # no static launch of 64 is timed: between the two (the step is hop-bound)

    # ---- sessions ----
    print("# session: one T2SSession over the queue; admit = median ms by rows admitted; adopt = median us / byte floor us of the "
          "largest admission; relaunch = median (advance wall - chunk * in-launch step) us")
    rows = [dict(x=xs[i], bert=berts[i], prompt=prompts[i], key=keys[i], force=force[i]) for i in range(n)]
    for slots in a.slots:
        for chunk in a.chunks:
            for admit_min in sorted({1, max(1, slots // 8), slots // 4, slots // 2}):
                times, occ, admits, adopts, relaunch = [], [], {}, [], []
                for rep in range(a.reps + 1):
                    sync()
                    t0 = time.perf_counter()
                    got, q, slot_steps = {}, 0, 0
                    with eng.open_session(slots, force=True, **kw) as ses:
                        where = {}
                        while q < n or ses.live:
                            k = admit_count(len(ses.free), n - q, ses.live, admit_min)
                            if k:
                                ta = time.perf_counter()
                                for t, i in zip(ses.admit(rows[q:q + k]), range(q, q + k)):
                                    where[t] = i
                                if rep:
                                    admits.setdefault(k, []).append((time.perf_counter() - ta) * 1e3)
                                q += k
                            ta = time.perf_counter()
                            done = ses.advance(chunk)
                            if rep:
                                relaunch.append(((time.perf_counter() - ta) * 1e3 - chunk * step_ms[slots if slots in step_ms else 128]) * 1e3)
                            slot_steps += slots * chunk
                            for t, y, idx in done:
                                got[where[t]] = idx
                        assert set(ses.modes) == {1}, "every advance must run on the persistent engine"
                        if rep:
                            adopts += ses.adopt
                    sync()
                    assert [got[i] for i in range(n)] == lens
                    if rep:
                        times.append((time.perf_counter() - t0) * 1e3)
                        occ.append(tokens / slot_steps)
                big = max(admits)
                ad = [(ms, nb) for k, ms, nb in adopts if k == big]
                floor_us = med([2 * nb / HBM * 1e6 for _, nb in ad])
                adm = " ".join(f"{k}:{med(v):.2f}" for k, v in sorted(admits.items()) if k in (1, big) or len(v) >= a.reps)
                print(f"{'session':>8} {slots:>4} {chunk:>5} {admit_min:>9} {med(times):>9.1f} {tokens / med(times) * 1e3:>9.0f} "
                      f"{med(occ):>9.3f}   admit ms {{{adm}}}  adopt[{big} rows] {med([ms for ms, _ in ad]) * 1e3:.0f} / "
                      f"{floor_us:.0f} us  relaunch {med(relaunch):.0f} us", flush=True)


if __name__ == "__main__":
    main()
