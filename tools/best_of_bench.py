#!/usr/bin/env python3
"""Cost of "best_of" candidates and of the per-token log-probabilities they are scored by (measurement tool, not product
code; not part of bench.py).

fp16, the full-size synthetic v2 pipeline of bench.py (80 phonemes, 100 prompt tokens, 100 generated tokens = 4 s per
sentence; the synthetic weights never emit EOS, so every row runs to the early stop and every candidate is "cut"), top_k = 15.
In one process, medians of --reps (7) calls after 2 warm-up calls each:

  pipeline   TTS.run of 8 sentences with best_of 1 / 2 / 4 and of 32 sentences with best_of 1 / 4: the AR stage (run()'s own
             stage clock) and the whole call, host clock, ms;
  step       the decode of B = 32 (one quad per group) and B = 128 rows (pipelined quads) with log-probabilities off and on:
             device ms per step of the persistent launch (gsv_t2s_decode_info), i.e. the default kernels against the LOGP
             kernels of csrc/t2s_mega.hip.

    python tools/best_of_bench.py > profiles/best_of_bench.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gpt-sovits_amd"))
import torch  # noqa: E402

from gsv import synthetic as S  # noqa: E402

DEV = "cuda:0"
TOK = 100


def med(v):
    return statistics.median(v)


def build():
    from gsv.TTS_infer_pack.TTS import TTS
    t2s_cfg = {k: dict(v) for k, v in S.T2S_V2_CONFIG.items()}
    t2s_cfg["data"]["max_sec"] = TOK / 50.0
    tts = TTS({"device": DEV, "is_half": True, "version": "v2", "max_batch": 128, "max_seq": 80 + 100 + TOK + 16})
    tts.init_t2s_weights(state={"weight": S.make_t2s_state_dict(S.T2S_V2_CONFIG, seed=0, suppress_eos=True), "config": t2s_cfg})
    tts.init_vits_weights(state={"weight": S.make_vits_state_dict(S.VITS_V2_CONFIG, seed=0), "config": dict(S.VITS_V2_CONFIG)})
    return tts


def segments(n):
    utt = S.make_utterances(n, seed=0)
    segs = [{"phones": it["phones"], "bert_features": torch.zeros(1024, len(it["phones"])), "norm_text": it["norm_text"]}
            for it in utt["items"]]
    return utt, segs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    tts = build()
    utt, segs = segments(32)
    tts.set_prompt_cache(utt["prompt_semantic"], [S.make_refer_spec().to(DEV)], phones=utt["prompt_phones"],
                         bert_features=torch.zeros(1024, len(utt["prompt_phones"])), norm_text="x" * 40)
    base = dict(top_k=15, top_p=1.0, temperature=1.0, repetition_penalty=1.35, seed=0, split_bucket=True, parallel_infer=True,
                fragment_interval=0.3)
    print(f"# best_of: fp16 synthetic v2, {TOK} tokens per sentence, top_k 15, medians of {a.reps}")
    print("# sentences best_of rows  AR_ms  end_to_end_ms  tokens_kept")
    for n, best_ofs in ((8, (1, 2, 4)), (32, (1, 4))):
        for k in best_ofs:
            req = dict(base, segments=segs[:n], batch_size=n, **({"best_of": k} if k > 1 else {}))
            ar, e2e = [], []
            for i in range(2 + a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = list(tts.run(dict(req)))
                torch.cuda.synchronize()
                if i >= 2:
                    e2e.append(1e3 * (time.perf_counter() - t0))
                    ar.append(1e3 * tts.last_timing[2])
            assert len(out) == 1 and out[0][1].size > 0
            print(f"{n:10d} {k:7d} {n * k:4d} {med(ar):6.1f} {med(e2e):14.1f} {tts.last_generated_tokens:12d}")
    print("# decode step, persistent engine: device ms per step (launch of 99 steps), log-probabilities off / on")
    print("#    B  off_ms_per_step  on_ms_per_step  on/off")
    eng = tts.t2s_model
    m = S.T2S_V2_CONFIG["model"]
    for B in (32, 128):
        xs = [torch.from_numpy(S.hash_ints(f"bo_x{i}", 80, m["phoneme_vocab_size"], 0)).long().to(DEV) for i in range(B)]
        berts = [torch.zeros(1024, 80) for _ in range(B)]
        prompts = torch.from_numpy(S.hash_ints("bo_p", 100, m["vocab_size"] - 1, 0)).long().to(DEV).view(1, -1).expand(B, -1)
        kw = dict(top_k=15, top_p=1.0, temperature=1.0, early_stop_num=TOK - 1, repetition_penalty=1.35, seed=0)
        per = {}
        for on in (False, True, False, True):
            t = []
            for i in range(2 + a.reps):
                eng.infer_panel_batch_infer(xs, None, prompts, berts, logprobs=on, **kw)
                mode, ms, steps = eng.decode_info()
                assert mode == 1 and steps > 0, "the persistent engine must run"
                if i >= 2:
                    t.append(ms / steps)
            per.setdefault(on, []).append(med(t))
        off, on_ = min(per[False]), min(per[True])
        print(f"{B:6d} {off:16.4f} {on_:15.4f} {on_ / off:7.3f}    # both passes: off {per[False]}, on {per[True]}")


if __name__ == "__main__":
    main()
