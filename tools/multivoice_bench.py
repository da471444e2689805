"""Multi-voice throughput: N requests, each with its own reference voice (prompt length, spectrogram), one 4 s sentence
each, fp16 synthetic v2 weights.  TTS.run_batch (one shared AR decode) against N sequential TTS.run calls (one voice per
call, the only way before run_batch).  Prints one JSON line: audio-s/s of both, the speed-up, and the persistent engine's
fallback count (gsv_t2s_engine_stats), which must stay 0.  --shared-sovits also times run_batch(shared_sovits=True) (one
segmented SoVITS pass for all voices) in the same process and reports its SoVITS device time.  Every mode lists the wall
time of each iteration, so the gain can be read against the spread.  --mixed-sampling spreads the requests evenly over four
(top_k, top_p, temperature) settings and times run_batch() against run_batch(mixed_sampling=True) only (both with
shared_sovits when --shared-sovits is given): ms per call, AR launches per call and AR wall time per call of both.

    python tools/multivoice_bench.py [--requests 32] [--tokens 100] [--iters 3] [--shared-sovits] [--mixed-sampling]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gpt-sovits_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=100, help="AR tokens per request (25 tokens = 1 s)")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--shared-sovits", action="store_true", help="also time run_batch(shared_sovits=True)")
    ap.add_argument("--mixed-sampling", action="store_true",
                    help="four sampling settings over the requests: run_batch() against run_batch(mixed_sampling=True)")
    a = ap.parse_args()
    from bench import build_tts, make_segments
    from gsv import synthetic as S
    dev = torch.device("cuda:0")
    N, TOK = a.requests, a.tokens
    tts = build_tts(dev, TOK, N, dtype_half=True)
    tts.configs.max_seq = 80 + 160 + TOK + 16          # room for the longest voice's prompt
    tts.t2s_model = None
    tts.init_t2s_weights(tts.configs.t2s_weights_path, state=tts._t2s_state)
    utt, segs = make_segments(N)
    voices = []
    for i in range(N):
        P = 60 + (i * 37) % 100                        # prompt lengths 60..159
        n_ph = len(utt["prompt_phones"])
        voices.append(tts.make_voice(torch.from_numpy(S.hash_ints(f"mv_sem{i}", P, 1024, 1)),
                                     [S.make_refer_spec(frames=150 + 7 * i, seed=100 + i).to(dev).half()],
                                     phones=S.hash_ints(f"mv_ph{i}", n_ph, 732, 1).tolist(),
                                     bert_features=torch.zeros(1024, n_ph), norm_text="x" * n_ph))
    params = dict(top_k=15, top_p=1.0, temperature=1.0, repetition_penalty=1.35, fragment_interval=0.01, seed=7)
    reqs = [dict(params, segments=[segs[i]], voice=voices[i]) for i in range(N)]

    times = {}

    def audio_s(outs):
        return sum(int(w.shape[0]) for _sr, w in outs) / 32000.0

    def timed(fn):
        best, each = None, []
        for it in range(a.iters + 1):                  # first pass: warm-up (graphs, workspaces)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
            if it > 0:
                each.append(round(dt, 4))
        times[fn] = each
        return outs, best

    def sequential():
        outs = []
        for r in reqs:
            v = r["voice"]
            tts.set_prompt_cache(v["prompt_semantic"], [s for s, _ in v["refer_spec"]], phones=v["phones"],
                                 bert_features=v["bert_features"], norm_text=v["norm_text"])
            outs += list(tts.run({k: x for k, x in r.items() if k != "voice"}))
        return outs

    def batch():
        return tts.run_batch(reqs)

    def batch_shared():
        return tts.run_batch(reqs, shared_sovits=True)

    if a.mixed_sampling:
        four = [(15, 1.0, 1.0), (5, 1.0, 0.8), (30, 0.9, 1.0), (0, 0.8, 1.2)]
        for i, r in enumerate(reqs):
            r["top_k"], r["top_p"], r["temperature"] = four[i * 4 // N]
        ar = {"launches": 0, "s": 0.0}
        run = tts.t2s_model._run

        def counted(*args, **kw):
            t0 = time.perf_counter()                       # _run returns the ids on the host: the wall time covers the decode
            out = run(*args, **kw)
            ar["launches"] += 1
            ar["s"] += time.perf_counter() - t0
            return out

        tts.t2s_model._run = counted
        res = {"requests": N, "tokens_per_request": TOK, "settings": four, "shared_sovits": bool(a.shared_sovits)}
        outs = {}
        for name, mixed in (("split", False), ("mixed", True)):
            fn = lambda mixed=mixed: tts.run_batch(reqs, shared_sovits=a.shared_sovits, mixed_sampling=mixed)  # noqa: E731
            ar["launches"], ar["s"] = 0, 0.0
            outs[name], best = timed(fn)
            res.update({f"{name}_ms_per_call": round(best * 1e3, 2), f"{name}_iters_s": times[fn],
                        f"{name}_ar_launches_per_call": ar["launches"] // (a.iters + 1),
                        f"{name}_ar_ms_per_call_mean": round(ar["s"] * 1e3 / (a.iters + 1), 2)})
        res["outputs_identical"] = f"{sum(int(x[1].shape == y[1].shape and (x[1] == y[1]).all()) for x, y in zip(outs['split'], outs['mixed']))}/{N}"
        res["ar_ratio_split_over_mixed"] = round(res["split_ar_ms_per_call_mean"] / res["mixed_ar_ms_per_call_mean"], 2)
        res["engine_fallbacks"], res["decode_mode"] = tts.t2s_model.engine_stats()[1], tts.t2s_model.decode_info()[0]
        print(json.dumps(res))
        return
    so, st = timed(sequential)
    bo, bt = timed(batch)
    _avail, fallbacks, _err = tts.t2s_model.engine_stats()
    same = sum(int(x[1].shape == y[1].shape and (x[1] == y[1]).all()) for x, y in zip(so, bo))
    res = {"requests": N, "tokens_per_request": TOK,
           "sequential_audio_s_per_s": round(audio_s(so) / st, 1), "run_batch_audio_s_per_s": round(audio_s(bo) / bt, 1),
           "speedup": round(st / bt, 2), "sequential_s": round(st, 4), "run_batch_s": round(bt, 4),
           "outputs_identical": f"{same}/{N}", "engine_fallbacks": fallbacks, "decode_mode": tts.t2s_model.decode_info()[0]}
    res["sequential_iters_s"], res["run_batch_iters_s"] = times[sequential], times[batch]
    if a.shared_sovits:
        n0 = tts.vits_model.decode_segments_calls
        ho, ht = timed(batch_shared)
        dev_ms, gen_ms = tts.vits_model.last_timing()      # of the last pass of the last iteration
        res.update({"shared_audio_s_per_s": round(audio_s(ho) / ht, 1), "shared_s": round(ht, 4), "shared_iters_s": times[batch_shared],
                    "shared_speedup_over_run_batch": round(bt / ht, 2),
                    "shared_passes_per_call": (tts.vits_model.decode_segments_calls - n0) // (a.iters + 1),
                    "shared_sovits_device_ms": round(dev_ms, 2), "shared_sovits_generator_ms": round(gen_ms, 2),
                    "shared_equal_lengths": f"{sum(int(x[1].shape == y[1].shape) for x, y in zip(bo, ho))}/{N}",
                    "engine_fallbacks": tts.t2s_model.engine_stats()[1]})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
