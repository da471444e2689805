"""LoRA voices beside the base model: 32 requests of one ~4 s sentence, fp16, the full-size synthetic v3 model of
tools/multivoice_v3_bench.py, sample_steps = 32, rank-32 adapters, over V in {1, 4, 32} fine-tuned voices (request i uses
voice i mod V; every request keeps its own reference audio).  Per V, in one process:

  (a) run_batch(shared_cfm=True) with the key "lora_voice" (TTS.add_lora_voice: all voices in the shared flow-matching passes);
  (b) the same requests without the key: (a) - (b) is what the two delta launches per DiT block cost, reported as ms per row
      and Euler step next to (b)'s own ms per row and Euler step;
  (c) what serving these voices takes without the feature: per voice init_vits_weights(state=lora, base_state=base) (the
      merge, the upload and the re-pack of the whole model, timed on its own) and then run_batch(shared_cfm=True) of that
      voice's requests.  At most --merge-voices voices are reloaded (each reload moves 0.7 GB); the figures say how many.

Prints one JSON line; every mode lists the wall time of each iteration after one warm-up call.

    python tools/lora_voices_bench.py [--voices 1,4,32] [--requests 32] [--rank 32] [--iters 3] [--merge-voices 4]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gpt-sovits_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from multivoice_v3_bench import build_v3, spread  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voices", default="1,4,32")
    ap.add_argument("--requests", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=100, help="AR tokens per request (25 tokens = 1 s)")
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--merge-voices", type=int, default=4)
    a = ap.parse_args()
    from bench import make_segments
    from gsv import synthetic as S
    dev = torch.device("cuda:0")
    N = a.requests
    tts = build_v3(dev, a.tokens, N)
    base_state = tts._vits_state
    vsd, vcfg = base_state["weight"], base_state["config"]
    utt, segs = make_segments(N)
    n_ph = len(utt["prompt_phones"])
    refs = []
    for i in range(N):
        P, Tm = 60 + (i * 37) % 100, 200 + (i * 53) % 400
        refs.append(tts.make_voice(torch.from_numpy(S.hash_ints(f"mv3_sem{i}", P, 1024, 1)),
                                   [S.make_refer_spec(frames=150 + 7 * i, seed=100 + i).to(dev)],
                                   phones=S.hash_ints(f"mv3_ph{i}", n_ph, 732, 1).tolist(), bert_features=torch.zeros(1024, n_ph),
                                   norm_text="x" * n_ph, ref_mel=S.hash_symmetric(f"mv3_mel{i}", (1, 100, Tm), 5.0, 3) - 5.0))
    params = dict(top_k=15, top_p=1.0, temperature=1.0, repetition_penalty=1.35, fragment_interval=0.01, seed=7, sample_steps=a.steps)
    plain = [dict(params, segments=[segs[i]], voice=refs[i]) for i in range(N)]
    sr = tts.vocoder_configs["sr"]

    def timed(fn):
        each, outs = [], None
        for it in range(a.iters + 1):                    # first pass: warm-up (workspaces)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs = fn()
            torch.cuda.synchronize()
            if it > 0:
                each.append(time.perf_counter() - t0)
        return outs, each

    def record(outs, each):
        audio = sum(int(w.shape[0]) for _sr, w in outs) / float(sr)
        med = statistics.median(each)
        return {"audio_s": round(audio, 2), "ms_per_call": round(med * 1e3, 1), "audio_s_per_s": round(audio / med, 1), "call_s": spread(each)}

    rows = []
    inner = tts.vits_model.cfm.inference_rows

    def spy(mu, prompts, *x, **k):
        rows.append(int(mu.shape[0]))
        return inner(mu, prompts, *x, **k)
    res = {"requests": N, "tokens_per_request": a.tokens, "sample_steps": a.steps, "rank": a.rank, "dtype": "f16", "by_voices": {}}
    for V in [int(v) for v in a.voices.split(",")]:
        states = [{"weight": S.make_lora_state_dict(vsd, rank=a.rank, seed=50 + v), "config": vcfg, "lora_rank": a.rank} for v in range(V)]
        free0 = torch.cuda.mem_get_info()[0]
        t0 = time.perf_counter()
        for v in range(V):
            tts.add_lora_voice(f"v{v}", state=states[v])
        torch.cuda.synchronize()
        add_ms = (time.perf_counter() - t0) * 1e3 / V
        added_mb = (free0 - torch.cuda.mem_get_info()[0]) / 2 ** 20
        keyed = [dict(r, lora_voice=f"v{i % V}") for i, r in enumerate(plain)]
        tts.vits_model.cfm.inference_rows = spy
        del rows[:]
        ao, ae = timed(lambda: tts.run_batch(keyed, shared_cfm=True))
        n_rows = sum(rows) // (a.iters + 1)
        bo, be = timed(lambda: tts.run_batch(plain, shared_cfm=True))
        tts.vits_model.cfm.inference_rows = inner
        for v in range(V):
            tts.remove_lora_voice(f"v{v}")
        d_ms = (statistics.median(ae) - statistics.median(be)) * 1e3
        out = {"with_key": record(ao, ae), "without_key": record(bo, be), "cfm_rows_per_call": n_rows,
               "add_lora_voice_ms_per_voice": round(add_ms, 1), "device_memory_added_mb": round(added_mb, 1),
               "delta_ms_per_row_and_step": round(d_ms / (n_rows * a.steps), 4),
               "call_ms_per_row_and_step_without_key": round(statistics.median(be) * 1e3 / (n_rows * a.steps), 4)}
        # (c) one merged model per voice, reloaded before its requests
        M = min(V, a.merge_voices)
        reload_ms, run_s = [], []
        for v in range(M):
            mine = [plain[i] for i in range(N) if i % V == v]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tts.init_vits_weights(state=states[v], base_state=base_state)
            torch.cuda.synchronize()
            reload_ms.append((time.perf_counter() - t0) * 1e3)
            _, each = timed(lambda: tts.run_batch(mine, shared_cfm=True))
            run_s.append(statistics.median(each))
        tts.init_vits_weights(state=base_state)
        inner = tts.vits_model.cfm.inference_rows
        out["merged_per_voice"] = {"voices_measured": M, "of": V, "reload_ms_each": [round(x, 1) for x in reload_ms],
                                   "run_batch_ms_each": [round(x * 1e3, 1) for x in run_s],
                                   "requests_per_voice": N // V + (1 if N % V else 0)}
        res["by_voices"][str(V)] = out
        del states
    print(json.dumps(res))


if __name__ == "__main__":
    main()
