#!/usr/bin/env python3
"""v2Pro voice enrolment, the speaker embedding: the per-audio loop (`SV.compute_embedding3` once per reference audio, what
`set_ref_audio` / `make_voice` do; unchanged by the packed pass, hence the parent commit's cost) against one
`SV.compute_embedding3_many` call over the same audios, in the same process, alternating.  Full-size synthetic
ERes2NetV2(24, 4, 4).  Steps, each a child process of its own under its own time limit (a step that fails or runs out of time
ends the run: nothing more is started on the device):

  table     1 / 8 / 32 audios of 3 / 6 / 10 s, medians of --reps runs after --warmup runs, host wall clock around work that ends
            in a device synchronise
  sweep     `max_frames` on the 32 x 10 s job: passes, time, peak workspace
  device    the device time of ONE per-audio encoder pass (forward3 on precomputed features) and of one packed pass: events around
            launches that were queued behind a long-running blocker, so the gaps the host leaves between launches are not in it;
            beside it the wall clock of the same pass issued on an idle device
  pipeline  32 x `TTS.make_voice` against `TTS.make_voices(shared_sv=True)` (and plain `make_voices`) on v2Pro WAV files of 6 s,
            fresh voice LRU each time

Measurement tool, not product code; not part of bench.py.

    python tools/sv_enrol_bench.py > profiles/sv_enrol.json          # prints one JSON line
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = {"table": 420, "sweep": 300, "device": 180, "pipeline": 420}             # seconds each child may take

ap = argparse.ArgumentParser()
ap.add_argument("--step", choices=sorted(STEPS), help="run one step in this process (what the parent starts)")
ap.add_argument("--steps", nargs="*", default=["table", "sweep", "device", "pipeline"])
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--counts", type=int, nargs="*", default=[1, 8, 32])
ap.add_argument("--seconds", type=float, nargs="*", default=[3, 6, 10])
ap.add_argument("--sweep", type=int, nargs="*", default=[1024, 2048, 4096, 8192, 16384, 32768])
ap.add_argument("--voices", type=int, default=32)
args = ap.parse_args()

if args.step is None:
    # the parent never opens the device: it starts one fresh child per step and stops at the first that does not end well
    out = {"tool": "sv_enrol_bench", "reps": args.reps}
    passthrough = ["--reps", str(args.reps), "--warmup", str(args.warmup), "--voices", str(args.voices),
                   "--counts", *map(str, args.counts), "--seconds", *map(str, args.seconds), "--sweep", *map(str, args.sweep)]
    for step in args.steps:
        cmd = ["timeout", "-k", "10", str(STEPS[step]), sys.executable, os.path.abspath(__file__), "--step", step] + passthrough
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            out[step] = {"failed": r.returncode}
            print(json.dumps(out))
            sys.exit(f"sv_enrol_bench: step {step} ended with status {r.returncode}; nothing more is run")
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))
    sys.exit(0)

sys.path.insert(0, os.path.join(HERE, "..", "gpt-sovits_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gsv import synthetic as S  # noqa: E402
from gsv.eres2net import kaldi as Kaldi  # noqa: E402
from gsv.eres2net.ERes2NetV2 import DEFAULT_MAX_FRAMES  # noqa: E402
from gsv.sv import SV  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("sv_enrol_bench needs the MI355X: there is no CPU path to time")
DEV = "cuda:0"
sv_sd = S.make_eres2net_state_dict(seed=0)


def audios(n, seconds):
    """n device waveforms of about `seconds` (lengths differ by a few hundred samples, as real files do)"""
    return [S.make_waveform(int(seconds * 16000) + 137 * k, 100 + k).to(DEV) for k in range(n)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def median_pair(a, b):
    """medians (ms) of a and b, run alternately, and the spread (max - min) of each"""
    for _ in range(args.warmup):
        a(); b()
    ta, tb = [], []
    for _ in range(args.reps):
        ta.append(timed(a)); tb.append(timed(b))
    return statistics.median(ta), statistics.median(tb), max(ta) - min(ta), max(tb) - min(tb)


def step_table():
    sv = SV(DEV, False, state_dict=sv_sd)
    net = sv.embedding_model
    rows = []
    for sec in args.seconds:
        for n in args.counts:
            ws = audios(n, sec)
            loop = lambda: [sv.compute_embedding3(w.unsqueeze(0)) for w in ws]
            many = lambda: sv.compute_embedding3_many(ws)
            p0, l0 = net.seg_passes, net.launches
            out = many()
            passes, launches = net.seg_passes - p0, net.launches - l0
            l0 = net.launches
            ref = loop()
            loop_launches = net.launches - l0
            diff = max(float((o - r).abs().max()) for o, r in zip(out, ref))
            tl, tm, sl, sm = median_pair(loop, many)
            rows.append({"audios": n, "seconds": sec, "frames": sum(1 + (int(w.numel()) - 400) // 160 for w in ws), "passes": passes,
                         "loop_launches": loop_launches, "packed_launches": launches,
                         "loop_ms": round(tl, 3), "packed_ms": round(tm, 3), "loop_spread_ms": round(sl, 3),
                         "packed_spread_ms": round(sm, 3), "speedup": round(tl / tm, 2), "max_abs_packed_vs_loop": float(f"{diff:.3g}")})
            del ws, out, ref
    return {"default_max_frames": DEFAULT_MAX_FRAMES, "device": torch.cuda.get_device_name(0), "rows": rows}


def step_sweep():
    sv = SV(DEV, False, state_dict=sv_sd)
    net = sv.embedding_model
    ws = audios(max(args.counts), max(args.seconds))
    points = []
    for mf in args.sweep:
        run = lambda: sv.compute_embedding3_many(ws, max_frames=mf)
        run()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        p0 = net.seg_passes
        run()
        torch.cuda.synchronize()
        passes, peak = net.seg_passes - p0, torch.cuda.max_memory_allocated() - base
        ta, tb, sa, sb = median_pair(run, run)
        points.append({"max_frames": mf, "passes": passes, "packed_ms": round(min(ta, tb), 3), "spread_ms": round(max(sa, sb), 3),
                       "peak_workspace_mb": round(peak / 2 ** 20, 1)})
    slot_frames = sum(p["frames"] for p in net.plan_segments([1 + (int(w.numel()) - 400) // 160 for w in ws], 1 << 30))
    return {"sweep": {"audios": len(ws), "seconds": max(args.seconds), "slot_frames": slot_frames, "points": points}}


def step_device():
    sv = SV(DEV, False, state_dict=sv_sd)
    net = sv.embedding_model
    big = torch.randn(8192, 8192, device=DEV)

    def blocker():
        for _ in range(12):                                     # tens of milliseconds of device work: the pass queues up behind it
            torch.mm(big, big)

    def queued(fn):
        """median device time of fn's launches, all of them in the queue before the first one starts"""
        ts = []
        for _ in range(args.warmup + args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            blocker()
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return statistics.median(ts[args.warmup:])

    rows = []
    for sec in args.seconds:
        w = audios(1, sec)[0]
        feat = Kaldi.fbank(w.unsqueeze(0), num_mel_bins=80, sample_frequency=16000, dither=0).unsqueeze(0)
        one = lambda: net.forward3(feat)
        l0 = net.launches
        one()
        launches = net.launches - l0
        wall, _, spread, _ = median_pair(one, one)
        rows.append({"pass": "per-audio", "audios": 1, "seconds": sec, "frames": int(feat.shape[1]), "launches": launches,
                     "device_ms": round(queued(one), 3), "wall_ms": round(wall, 3), "wall_spread_ms": round(spread, 3)})
    for n, sec in ((8, 6), (32, 6)):
        ws = audios(n, sec)
        feats = [Kaldi.fbank(w.unsqueeze(0), num_mel_bins=80, sample_frequency=16000, dither=0) for w in ws]
        many = lambda: net.forward3_segments(feats, max_frames=1 << 20)
        l0 = net.launches
        many()
        launches = net.launches - l0
        wall, _, spread, _ = median_pair(many, many)
        rows.append({"pass": "packed", "audios": n, "seconds": sec, "frames": sum(int(f.shape[0]) for f in feats), "launches": launches,
                     "device_ms": round(queued(many), 3), "wall_ms": round(wall, 3), "wall_spread_ms": round(spread, 3)})
    return {"device_time": rows}


def step_pipeline():
    import copy
    import tempfile
    import wave
    from gsv.TTS_infer_pack.TTS import TTS
    cfg = copy.deepcopy(S.VITS_V2_CONFIG)
    cfg["model"]["version"], cfg["model"]["gin_channels"] = "v2Pro", 1024
    tts = TTS({"device": DEV, "is_half": True, "version": "v2Pro", "max_batch": 4, "max_seq": 600})
    tts.init_t2s_weights(state={"weight": S.make_t2s_state_dict(S.T2S_V2_CONFIG, seed=0, suppress_eos=True), "config": S.T2S_V2_CONFIG})
    tts.init_vits_weights(state={"weight": S.make_vits_state_dict(cfg, seed=0), "config": cfg})
    tts.init_cnhuhbert_weights(state_dict=S.make_hubert_state_dict(seed=0))
    tts.init_sv_model(state_dict=sv_sd)
    with tempfile.TemporaryDirectory() as d:
        specs = []
        for k in range(args.voices):
            p = os.path.join(d, f"v{k}.wav")
            wav = S.make_waveform(6 * 32000 + 411 * k, 200 + k, sr=32000).numpy()
            with wave.open(p, "wb") as f:
                f.setnchannels(1); f.setsampwidth(2); f.setframerate(32000)
                f.writeframes((np.clip(wav, -1, 1) * 32767).astype("<i2").tobytes())
            specs.append({"ref_audio_path": p})

        def fresh():
            tts.__dict__.pop("_voice_lru", None)

        def one_by_one():
            fresh()
            return [tts.make_voice(**sp) for sp in specs]

        def hubert_only():
            fresh()
            return tts.make_voices(specs)

        def together():
            fresh()
            return tts.make_voices(specs, shared_sv=True)

        net = tts.sv_model.embedding_model
        p0 = net.seg_passes
        together()
        passes = net.seg_passes - p0
        t1, tm, s1, sm = median_pair(one_by_one, together)
        th, _, sh, _ = median_pair(hubert_only, hubert_only)
    return {"pipeline": {"voices": args.voices, "seconds": 6, "sv_passes": passes, "make_voice_x_n_ms": round(t1, 3),
                         "make_voices_shared_sv_ms": round(tm, 3), "make_voice_spread_ms": round(s1, 3),
                         "make_voices_shared_sv_spread_ms": round(sm, 3), "make_voices_plain_ms": round(th, 3),
                         "make_voices_plain_spread_ms": round(sh, 3), "speedup_vs_make_voice": round(t1 / tm, 2),
                         "speedup_vs_make_voices_plain": round(th / tm, 2)}}


print(json.dumps({"table": step_table, "sweep": step_sweep, "device": step_device, "pipeline": step_pipeline}[args.step]()))
