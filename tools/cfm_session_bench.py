"""Flow-matching sessions on the full-size synthetic v3 model, fp16 (DiT 1024 x 22, BigVGAN-v2, as tools/multivoice_v3_bench.py
builds them); medians of --iters timed calls after one warm-up call, every mode in the same process, the modes of a comparison
alternating call by call.  Prints one JSON line per section.

    python tools/cfm_session_bench.py [--iters 7] [--sections mixed,guided,uniform,slices,admit]

mixed    32 requests x ~4 s, each with its own voice, sample_steps in equal thirds of 8 / 16 / 32: run_batch(shared_cfm=True)
         (one pass per (sample_steps, rate) group) against run_batch(shared_cfm=True, continuous_cfm=True) (one session): ms per
         call, audio-s/s, DiT row-steps issued and mean live DiT rows per Euler step.
guided   the same with a third of the requests (four of each step count) guided at 0.7.
uniform  32 rows x 32 steps through a session (one admission, one step(32), 32 fetches) against CFM.inference_rows: what the
         per-row kernels, the gather and the packing cost.
slices   ms per row and Euler step with 8 / 16 / 32 live rows when 32 steps are taken as step(1) x 32, step(4) x 8, step(32).
admit    the cost of one admission of 1, 4 and 16 rows (step count already cached) into a session that has 8 live rows.
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


def med(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def alternate(modes, iters):
    """modes: {name: fn}; one warm-up round, then `iters` rounds, the modes alternating -> ({name: last output}, {name: [s]})"""
    outs, each = {}, {m: [] for m in modes}
    for it in range(iters + 1):
        for m, fn in modes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[m] = fn()
            torch.cuda.synchronize()
            if it:
                each[m].append(time.perf_counter() - t0)
    return outs, each


def requests_mix(tts, N, guided_every, dev):
    from bench import make_segments
    from gsv import synthetic as S
    utt, segs = make_segments(N)
    n_ph = len(utt["prompt_phones"])
    reqs = []
    for i in range(N):
        P, Tm = 60 + (i * 37) % 100, 200 + (i * 53) % 400
        voice = tts.make_voice(torch.from_numpy(S.hash_ints(f"mv3_sem{i}", P, 1024, 1)), [S.make_refer_spec(frames=150 + 7 * i, seed=100 + i).to(dev)],
                               phones=S.hash_ints(f"mv3_ph{i}", n_ph, 732, 1).tolist(), bert_features=torch.zeros(1024, n_ph),
                               norm_text="x" * n_ph, ref_mel=S.hash_symmetric(f"mv3_mel{i}", (1, 100, Tm), 5.0, 3) - 5.0)
        reqs.append(dict(top_k=15, top_p=1.0, temperature=1.0, repetition_penalty=1.35, fragment_interval=0.01, seed=7, segments=[segs[i]],
                         voice=voice, sample_steps=(8, 16, 32)[i % 3],
                         inference_cfg_rate=0.7 if guided_every and (i // 3) % guided_every == 0 else 0))
    return reqs


def mixed_section(tts, a, dev, guided_every, name):
    import gsv.TTS_infer_pack.TTS as M
    reqs = requests_mix(tts, a.requests, guided_every, dev)
    sr = tts.vocoder_configs["sr"]
    cfm = tts.vits_model.cfm
    passes, plans = [], []
    inner_rows, inner_plan = cfm.inference_rows, M.plan_cfm_session

    def spy_rows(mu, prompts, n, *x, **k):
        passes.append((int(mu.shape[0]), int(n), 2 if M.cfg_guided(k.get("inference_cfg_rate", 0)) else 1))
        return inner_rows(mu, prompts, n, *x, **k)

    def spy_plan(rows, cap):
        sched = inner_plan(rows, cap)
        plans.append((list(rows), sched))
        return sched
    cfm.inference_rows, M.plan_cfm_session = spy_rows, spy_plan
    try:
        outs, each = alternate({"grouped": lambda: tts.run_batch(reqs, shared_cfm=True),
                                "session": lambda: tts.run_batch(reqs, shared_cfm=True, continuous_cfm=True)}, a.iters)
    finally:
        cfm.inference_rows, M.plan_cfm_session = inner_rows, inner_plan
    res = {"section": name, "requests": a.requests, "iters": a.iters, "cfm_max_rows": tts.cfm_max_rows}
    for m in ("grouped", "session"):
        audio = sum(int(w.shape[0]) for _sr, w in outs[m]) / float(sr)
        s = statistics.median(each[m])
        res[m] = {"ms_per_call": round(s * 1e3, 1), "audio_s": round(audio, 2), "audio_s_per_s": round(audio / s, 1), "call_s": med(each[m])}
    per = passes[:len(passes) // (a.iters + 1)]
    steps = sum(n for _, n, _ in per)
    res["grouped"].update(passes=[(b, n, g) for b, n, g in per], dit_row_steps=sum(b * n * g for b, n, g in per),
                          euler_steps=steps, mean_live_dit_rows_per_step=round(sum(b * n * g for b, n, g in per) / max(1, steps), 2))
    rows, sched = plans[0]
    live, row_steps, steps = {}, 0, 0
    for admit, k in sched:
        for i in admit:
            live[i] = rows[i][0]
        row_steps += k * sum(2 if rows[i][1] else 1 for i in live)
        steps += k
        live = {i: n - k for i, n in live.items() if n > k}
    res["session"].update(admissions=sum(1 for ad, _ in sched if ad), step_calls=len(sched), dit_row_steps=row_steps, euler_steps=steps,
                          mean_live_dit_rows_per_step=round(row_steps / max(1, steps), 2))
    res["equal_lengths"] = f"{sum(int(x[1].shape == y[1].shape) for x, y in zip(outs['grouped'], outs['session']))}/{a.requests}"
    res["speedup_session_over_grouped"] = round(statistics.median(each["grouped"]) / statistics.median(each["session"]), 3)
    print(json.dumps(res), flush=True)


def rows_inputs(tts, B, dev):
    from gsv import synthetic as S
    T = tts.vocoder_configs["T_chunk"]
    mu = S.hash_symmetric("csb_mu", (B, T, 512), 1.0, B).to(dev).half()
    pr = [S.hash_symmetric("csb_p", (1, 100, 200 + (b * 67) % 269), 1.0, b).to(dev).half() for b in range(B)]
    return T, mu, pr, list(range(1, B + 1))


def uniform_section(tts, a, dev):
    cfm = tts.vits_model.cfm
    B, N = 32, 32
    T, mu, pr, seeds = rows_inputs(tts, B, dev)

    def session():
        with cfm.open_session(B, T) as s:
            slots = s.admit(mu, pr, N, 0.0, seeds=seeds)
            s.step(N)
            return torch.stack([s.fetch(sl) for sl in slots])
    outs, each = alternate({"inference_rows": lambda: cfm.inference_rows(mu, pr, N, seeds=seeds), "session": session}, a.iters)
    res = {"section": "uniform", "rows": B, "steps": N, "iters": a.iters,
           # inference_rows returns mu's dtype (fp16 here), fetch returns the fp32 state: compare after the same rounding
           "bit_equal": bool(torch.equal(outs["inference_rows"], outs["session"].to(outs["inference_rows"].dtype)))}
    for m in each:
        res[m] = {"ms_per_call": med([x * 1e3 for x in each[m]]), "ms_per_row_step": round(statistics.median(each[m]) * 1e3 / (B * N), 4)}
    print(json.dumps(res), flush=True)


def slices_section(tts, a, dev):
    cfm = tts.vits_model.cfm
    N, out = 32, []
    for B in (8, 16, 32):
        T, mu, pr, seeds = rows_inputs(tts, B, dev)
        for k in (1, 4, 32):
            ts = []
            for it in range(a.iters + 1):
                with cfm.open_session(B, T) as s:
                    s.admit(mu, pr, N, 0.0, seeds=seeds)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(N // k):
                        s.step(k)
                    torch.cuda.synchronize()
                    if it:
                        ts.append((time.perf_counter() - t0) * 1e3)
            out.append({"live_rows": B, "step_k": k, "calls": N // k, "ms_32_steps": med(ts),
                        "ms_per_row_step": round(statistics.median(ts) / (B * N), 4)})
    print(json.dumps({"section": "slices", "iters": a.iters, "steps": N, "slices": out}), flush=True)


def admit_section(tts, a, dev):
    cfm = tts.vits_model.cfm
    N, live, out = 32, 8, []
    T, mu, pr, seeds = rows_inputs(tts, live + 16, dev)
    for n in (1, 4, 16):
        ts = []
        for it in range(a.iters + 1):
            with cfm.open_session(live + n, T) as s:
                s.admit(mu[:live], pr[:live], N, 0.0, seeds=seeds[:live])
                s.step(1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                s.admit(mu[live:live + n], pr[live:live + n], N, 0.0, seeds=seeds[live:live + n])
                torch.cuda.synchronize()
                if it:
                    ts.append((time.perf_counter() - t0) * 1e3)
        out.append({"admitted_rows": n, "live_rows": live, "ms": med(ts)})
    print(json.dumps({"section": "admit", "iters": a.iters, "admissions": out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=100, help="AR tokens per request (25 tokens = 1 s)")
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--sections", default="mixed,guided,uniform,slices,admit")
    a = ap.parse_args()
    from multivoice_v3_bench import build_v3
    dev = torch.device("cuda:0")
    tts = build_v3(dev, a.tokens, a.requests)
    want = a.sections.split(",")
    if "mixed" in want:
        mixed_section(tts, a, dev, 0, "mixed")
    if "guided" in want:
        mixed_section(tts, a, dev, 3, "guided")
    if "uniform" in want:
        uniform_section(tts, a, dev)
    if "slices" in want:
        slices_section(tts, a, dev)
    if "admit" in want:
        admit_section(tts, a, dev)


if __name__ == "__main__":
    main()
