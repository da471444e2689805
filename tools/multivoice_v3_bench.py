"""Multi-voice v3 throughput: N requests of one ~4 s sentence, each with its own reference voice (prompt tokens, spectrogram
and a prompt mel of its own length, some longer than T_ref), fp16, the full-size synthetic v3 model (DiT 1024 x 22 and
BigVGAN-v2 as tools/cfm_bench.py / bench.py build them), sample_steps = 32.  TTS.run_batch(shared_cfm=True) (the
flow-matching stage of all voices in shared passes) against TTS.run_batch() (one flow-matching pass per request) in the
same process, then the CFM alone: ms per Euler step of CFM.inference_rows at B = 8, 16, 32, 64 rows of T_chunk frames with
mixed prompt lengths.  Prints one JSON line; every mode lists the wall time of each iteration after one warm-up call, so a
gain can be read against the spread.

    python tools/multivoice_v3_bench.py [--requests 32] [--tokens 100] [--iters 3] [--plain-only] [--no-sweep] [--once]
    python tools/multivoice_v3_bench.py --shared-vocoder [--no-sweep] [--once]

--plain-only times run_batch() alone (also runs on a tree without shared_cfm); --once makes one shared call after the
warm-up and nothing else (the run a kernel trace is taken of).
--shared-vocoder: run_batch(shared_cfm=True, shared_vocoder=True) (all folds vocoded in shared segmented passes) against
run_batch(shared_cfm=True) (one vocoder call per fold) in the same process, timed calls alternating, with the vocoder
stage's own time per call under HIP events; then the sweep of frames per pass: forward_segments over segments of 600 frames
up to 1 k ... 32 k frames in all, ms per 1 k frames and the device memory the pass added.  On a tree without the keyword it
times run_batch(shared_cfm=True) alone (the parent's side of an alternating-process comparison).
"""
import argparse
import copy
import inspect
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


def build_v3(dev, tokens, batch):
    from gsv import synthetic as S
    from gsv.TTS_infer_pack.TTS import TTS
    t2s_cfg = {k: dict(v) for k, v in S.T2S_V2_CONFIG.items()}
    t2s_cfg["data"]["max_sec"] = tokens / 50.0
    tts = TTS({"device": str(dev), "is_half": True, "version": "v3", "max_batch": batch, "max_seq": 80 + 160 + tokens + 16})
    tts.init_t2s_weights(state={"weight": S.make_t2s_state_dict(S.T2S_V2_CONFIG, seed=0, suppress_eos=True), "config": t2s_cfg})
    vcfg = copy.deepcopy(S.VITS_V2_CONFIG)
    vcfg["model"]["version"] = "v3"
    dit = dict(S.DIT_V3_CONFIG)
    vsd = S.make_vits_v3_state_dict(vcfg, seed=0, dit_cfg=dit)
    vcfg["dit"] = {k: v for k, v in dit.items() if k != "mel_dim"}
    tts.init_vits_weights(state={"weight": vsd, "config": vcfg})
    ocfg = dict(S.BIGVGAN_V2_24K_CONFIG)
    tts.init_vocoder(state={"weight": S.make_vocoder_state_dict(ocfg, seed=4), "config": ocfg})
    return tts


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "each": [round(x, 4) for x in xs]}


class TimedVocoder:
    """the vocoder with HIP events around every call: ms[i] = (start, end) of call i on the current stream (the engine's
    stream waits for it and is synchronised before the call returns)"""

    def __init__(self, inner):
        self.inner, self.events = inner, []

    def _timed(self, fn, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn(*a)
        e1.record()
        self.events.append((e0, e1))
        return out

    def __call__(self, x):
        return self._timed(self.inner, x)

    def forward_segments(self, mels):
        return self._timed(self.inner.forward_segments, mels)

    def segment_gap(self):
        return self.inner.segment_gap()

    def take_ms(self):
        torch.cuda.synchronize()
        ms, self.events = sum(a.elapsed_time(b) for a, b in self.events), []
        return ms


def shared_vocoder_mode(a, tts, reqs, res, record, TTS):
    from gsv import synthetic as S
    has_kw = "shared_vocoder" in inspect.signature(TTS.run_batch).parameters
    voc = tts.vocoder = TimedVocoder(tts.vocoder)
    modes = {"run_batch_shared_cfm": dict(shared_cfm=True)}
    if has_kw:
        modes["run_batch_shared_vocoder"] = dict(shared_cfm=True, shared_vocoder=True)
    if a.once:
        kw = modes["run_batch_shared_vocoder" if has_kw else "run_batch_shared_cfm"]
        for _ in range(2):
            tts.run_batch(reqs, **kw)
            torch.cuda.synchronize()
        print(json.dumps(dict(res, mode="once", keywords=sorted(kw))))
        return
    outs, each, voc_ms, calls = {}, {m: [] for m in modes}, {m: [] for m in modes}, {}
    for it in range(a.iters + 1):                        # first round: warm-up; the modes alternate call by call
        for m, kw in modes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[m] = tts.run_batch(reqs, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            calls[m] = len(voc.events)
            ms = voc.take_ms()
            if it > 0:
                each[m].append(dt)
                voc_ms[m].append(ms)
    for m in modes:
        res[m] = dict(record(outs[m], each[m]), vocoder_calls_per_call=calls[m],
                      vocoder_stage_ms={"median": round(statistics.median(voc_ms[m]), 2), "min": round(min(voc_ms[m]), 2),
                                        "max": round(max(voc_ms[m]), 2)})
    if has_kw:
        x, y = outs["run_batch_shared_cfm"], outs["run_batch_shared_vocoder"]
        res["vocoder_max_frames"] = tts.vocoder_max_frames
        res["equal_lengths"] = f"{sum(int(p[1].shape == q[1].shape) for p, q in zip(x, y))}/{len(x)}"
        res["speedup_shared_vocoder_over_shared_cfm"] = round(statistics.median(each["run_batch_shared_cfm"]) /
                                                              statistics.median(each["run_batch_shared_vocoder"]), 3)
        if not a.no_sweep:
            sweep, seg = [], 600
            for cap in (1024, 2048, 4096, 8192, 16384, 32768):
                n = max(1, cap // seg)
                mels = [S.hash_symmetric("mv3_voc", (1, 100, seg), 2.0, i).to(tts.configs.device) for i in range(n)]
                free0 = torch.cuda.mem_get_info()[0]
                ts = []
                for it in range(a.iters + 1):            # first pass: warm-up (workspaces)
                    voc.forward_segments(mels)
                    ms = voc.take_ms()
                    if it:
                        ts.append(ms)
                grown = free0 - torch.cuda.mem_get_info()[0]
                ms = statistics.median(ts)
                sweep.append({"cap": cap, "segments": n, "frames": n * seg, "ms": round(ms, 2), "ms_per_1k_frames": round(ms * 1000 / (n * seg), 3),
                              "min_max_ms": [round(min(ts), 2), round(max(ts), 2)], "device_memory_added_mb": round(grown / 2 ** 20, 1)})
                del mels
            one = [S.hash_symmetric("mv3_voc", (1, 100, seg), 2.0, 0).to(tts.configs.device)]
            ts = []
            for it in range(a.iters + 1):
                voc(one[0])
                ts.append(voc.take_ms())
            res["single_forward_600_frames_ms"] = round(statistics.median(ts[1:]), 2)
            res["vocoder_frames_sweep"] = sweep
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=100, help="AR tokens per request (25 tokens = 1 s)")
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--shared-vocoder", action="store_true")
    a = ap.parse_args()
    from bench import make_segments
    from gsv import synthetic as S
    from gsv.TTS_infer_pack.TTS import TTS
    dev = torch.device("cuda:0")
    N = a.requests
    tts = build_v3(dev, a.tokens, N)
    utt, segs = make_segments(N)
    n_ph = len(utt["prompt_phones"])
    voices = []
    for i in range(N):
        P = 60 + (i * 37) % 100                          # prompt tokens 60..159: 225..596 feature frames
        Tm = 200 + (i * 53) % 400                        # prompt mel 200..599 frames: about a third above T_ref = 468
        voices.append(tts.make_voice(torch.from_numpy(S.hash_ints(f"mv3_sem{i}", P, 1024, 1)),
                                     [S.make_refer_spec(frames=150 + 7 * i, seed=100 + i).to(dev)],
                                     phones=S.hash_ints(f"mv3_ph{i}", n_ph, 732, 1).tolist(), bert_features=torch.zeros(1024, n_ph),
                                     norm_text="x" * n_ph, ref_mel=S.hash_symmetric(f"mv3_mel{i}", (1, 100, Tm), 5.0, 3) - 5.0))
    params = dict(top_k=15, top_p=1.0, temperature=1.0, repetition_penalty=1.35, fragment_interval=0.01, seed=7, sample_steps=a.steps)
    reqs = [dict(params, segments=[segs[i]], voice=voices[i]) for i in range(N)]
    sr = tts.vocoder_configs["sr"]
    has_shared = "shared_cfm" in inspect.signature(TTS.run_batch).parameters

    def timed(fn, iters):
        each, outs = [], None
        for it in range(iters + 1):                      # first pass: warm-up (workspaces, graphs)
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

    res = {"requests": N, "tokens_per_request": a.tokens, "sample_steps": a.steps, "dtype": "f16"}
    if a.shared_vocoder:
        return shared_vocoder_mode(a, tts, reqs, res, record, TTS)
    if a.once:
        tts.run_batch(reqs, shared_cfm=True)
        torch.cuda.synchronize()
        tts.run_batch(reqs, shared_cfm=True)
        torch.cuda.synchronize()
        print(json.dumps(dict(res, mode="once")))
        return
    po, pe = timed(lambda: tts.run_batch(reqs), a.iters)
    res["run_batch"] = record(po, pe)
    if has_shared and not a.plain_only:
        rows = []
        inner = tts.vits_model.cfm.inference_rows

        def spy(mu, prompts, *x, **k):
            rows.append((int(mu.shape[0]), min(int(p.shape[2]) for p in prompts), max(int(p.shape[2]) for p in prompts)))
            return inner(mu, prompts, *x, **k)
        tts.vits_model.cfm.inference_rows = spy
        so, se = timed(lambda: tts.run_batch(reqs, shared_cfm=True), a.iters)
        tts.vits_model.cfm.inference_rows = inner
        res["run_batch_shared_cfm"] = record(so, se)
        res["shared_passes_per_call"] = len(rows) // (a.iters + 1)
        res["shared_pass_rows_prompt_min_max"] = rows[:len(rows) // (a.iters + 1)]
        res["cfm_max_rows"] = tts.cfm_max_rows
        res["speedup_shared_over_run_batch"] = round(statistics.median(pe) / statistics.median(se), 2)
        res["equal_lengths"] = f"{sum(int(x[1].shape == y[1].shape) for x, y in zip(po, so))}/{N}"
        if not a.no_sweep:
            T = tts.vocoder_configs["T_chunk"]
            cfm, sweep = tts.vits_model.cfm, []
            for B in (8, 16, 32, 64):
                mu = S.hash_symmetric("mv3_mu", (B, T, 512), 1.0, B).to(dev).half()
                pr = [S.hash_symmetric("mv3_p", (1, 100, 200 + (b * 67) % 269), 1.0, b).to(dev).half() for b in range(B)]
                seeds = list(range(1, B + 1))
                _, each = timed(lambda: cfm.inference_rows(mu, pr, 8, seeds=seeds), a.iters)
                ms = statistics.median(each) * 1e3 / 8
                sweep.append({"rows": B, "ms_per_step": round(ms, 3), "ms_per_step_per_row": round(ms / B, 4),
                              "min_max_ms_per_step": [round(min(each) * 1e3 / 8, 3), round(max(each) * 1e3 / 8, 3)]})
                del mu, pr
            res["cfm_rows_sweep_8_steps"] = sweep
    print(json.dumps(res))


if __name__ == "__main__":
    main()
