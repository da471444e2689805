#!/usr/bin/env python3
"""Voice enrolment: the per-audio HuBERT loop (`HubertModel.__call__` once per reference audio, what `set_ref_audio` /
`make_voice` do; unchanged by the packed pass, hence the parent commit's cost) against one `HubertModel.batch` call over the same
audios, in the same process, alternating.  Full-size synthetic HuBERT-base; 1 / 8 / 32 audios of 3 / 6 / 10 s; then a sweep of
`max_samples` on the largest job, the segmented GroupNorm kernel alone at the default pass size against its HBM floor, and the
pipeline pair: 32 x `TTS.make_voice` against one `TTS.make_voices` on WAV files (v2 synthetic weights, fresh voice LRU each time),
with the host part (load + resample, timed alone) and the rest (device part) reported separately.  Times are host wall clock
around work that ends in a device synchronise, medians of --reps runs after --warmup runs (measurement tool, not product code;
not part of bench.py).

--device-frontend: only the front-end comparison of DESIGN.md section 4m, on --voices WAV files of 6 s at each of --rates: (a) host
load_wav alone, (b) host load + resample alone (the prompt's, as above, and with the spectrogram's second read and resampling),
(c) make_voices, (d) make_voices(device_frontend=True), (c) and (d) alternating, and (e) the resample launches alone by device
events against their byte floor (input + output at 6.3 TB/s).

    python tools/voice_enrol_bench.py > profiles/voice_enrol.json         # prints one JSON line
    python tools/voice_enrol_bench.py --device-frontend > profiles/device_frontend.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time
import wave

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpt-sovits_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gsv import _lib  # noqa: E402
from gsv import synthetic as S  # noqa: E402
from gsv.feature_extractor.cnhubert import CNHubert  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--counts", type=int, nargs="*", default=[1, 8, 32])
ap.add_argument("--seconds", type=float, nargs="*", default=[3, 6, 10])
ap.add_argument("--sweep", type=int, nargs="*", default=[2 ** 19, 2 ** 20, 2 ** 21, 2 ** 22, 2 ** 23])
ap.add_argument("--voices", type=int, default=32, help="WAV files of the pipeline pair (0: skip it)")
ap.add_argument("--device-frontend", action="store_true", help="only the host / device front-end comparison (DESIGN.md 4m)")
ap.add_argument("--rates", type=int, nargs="*", default=[32000, 44100], help="file rates of --device-frontend")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("voice_enrol_bench needs the MI355X: there is no CPU path to time")
DEV = "cuda:0"

hubert_sd = S.make_hubert_state_dict(seed=0)
hub = CNHubert(device=DEV, state_dict=hubert_sd)
m = hub.model


def audios(n, seconds):
    """n device waveforms of about `seconds` (lengths differ by a few hundred samples, as real files do)"""
    return [S.make_waveform(int(seconds * 16000) + 137 * k, 100 + k).to(DEV) for k in range(n)]


def loop(ws):
    return [m(w.unsqueeze(0))["last_hidden_state"] for w in ws]


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


def make_tts():
    from gsv.TTS_infer_pack.TTS import TTS
    tts = TTS({"device": DEV, "is_half": True, "version": "v2", "max_batch": 4, "max_seq": 600})
    tts.init_t2s_weights(state={"weight": S.make_t2s_state_dict(S.T2S_V2_CONFIG, seed=0, suppress_eos=True), "config": S.T2S_V2_CONFIG})
    tts.init_vits_weights(state={"weight": S.make_vits_state_dict(S.VITS_V2_CONFIG, seed=0), "config": dict(S.VITS_V2_CONFIG)})
    tts.init_cnhuhbert_weights(state_dict=hubert_sd)
    return tts


def write_wavs(d, n, sr):
    specs = []
    for k in range(n):
        p = os.path.join(d, f"v{sr}_{k}.wav")
        wav = S.make_waveform(6 * sr + 411 * k, 200 + k, sr=sr).numpy()
        with wave.open(p, "wb") as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(sr)
            f.writeframes((np.clip(wav, -1, 1) * 32767).astype("<i2").tobytes())
        specs.append({"ref_audio_path": p})
    return specs


def device_frontend_bench():
    from gsv import audio_io as A
    tts = make_tts()
    out = []
    with tempfile.TemporaryDirectory() as d:
        for sr in args.rates:
            specs = write_wavs(d, args.voices, sr)
            paths = [sp["ref_audio_path"] for sp in specs]
            sr_model = tts.configs.sampling_rate

            def fresh():
                tts.__dict__.pop("_voice_lru", None)

            def load_only():
                return [A.load_wav(p) for p in paths]

            def host_prompt():
                return [tts._prompt_wav16k(p) for p in paths]

            def host_all():                                   # what make_voices does on the host per voice: two reads, two rates
                for p in paths:
                    tts._prompt_wav16k(p)
                    raw, raw_sr = A.load_wav(p)
                    A.resample(raw[:1], raw_sr, sr_model)

            def host_path():
                fresh()
                return tts.make_voices(specs)

            def device_path():
                fresh()
                return tts.make_voices(specs, device_frontend=True)

            va, vb = host_path(), device_path()
            same = sum(bool(torch.equal(x["prompt_semantic"], y["prompt_semantic"])) for x, y in zip(va, vb))
            spec_diff = max(float((x["refer_spec"][0][0].float() - y["refer_spec"][0][0].float()).abs().max()) for x, y in zip(va, vb))
            ta, tb, sa, sb = median_pair(load_only, host_prompt)
            tball, _, sball, _ = median_pair(host_all, host_all)
            tc, td, sc, sd = median_pair(host_path, device_path)
            # (e) the resample launches alone, by device events
            raws = [A.load_wav(p)[0][0] for p in paths]
            stream = torch.from_numpy(np.concatenate(raws)).to(DEV)
            lens = [int(r.shape[0]) for r in raws]
            starts = [0] + list(np.cumsum(lens)[:-1])
            targets = sorted({16000, sr_model} - {sr})

            def launches():
                for t in targets:
                    A.resample_segments(stream, starts, lens, sr, t, peak=True)

            for _ in range(3):
                launches()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
            for a, b in ev:
                a.record(); launches(); b.record()
            torch.cuda.synchronize()
            e_ms = statistics.median(a.elapsed_time(b) for a, b in ev)
            e_bytes = sum(4 * (sum(lens) + sum(A.resampled_len(n, sr, t) for n in lens)) for t in targets)
            out.append({"file_rate": sr, "voices": args.voices, "seconds": 6, "a_load_wav_ms": round(ta, 3), "a_spread_ms": round(sa, 3),
                        "b_load_resample_prompt_ms": round(tb, 3), "b_spread_ms": round(sb, 3),
                        "b_load_resample_prompt_and_spec_ms": round(tball, 3), "b_all_spread_ms": round(sball, 3),
                        "c_make_voices_ms": round(tc, 3), "c_spread_ms": round(sc, 3),
                        "d_make_voices_device_frontend_ms": round(td, 3), "d_spread_ms": round(sd, 3),
                        "e_resample_launches": len(targets), "e_resample_ms": round(e_ms, 4), "e_bytes": e_bytes,
                        "e_floor_ms_at_6.3_tb_per_s": round(e_bytes / 6.3e9, 5),
                        "voices_with_equal_prompt_codes": same, "max_abs_spec_diff": round(spec_diff, 5)})
    return {"tool": "voice_enrol_bench --device-frontend", "device": torch.cuda.get_device_name(0), "reps": args.reps, "rates": out}


if args.device_frontend:
    print(json.dumps(device_frontend_bench()))
    sys.exit(0)

rows = []
for sec in args.seconds:
    for n in args.counts:
        ws = audios(n, sec)
        p0 = m.passes
        out = m.batch(ws)
        passes = m.passes - p0
        ref = loop(ws)
        diff = max(float((o.float() - r.float()).abs().max()) for o, r in zip(out, ref))
        tl, tb, sl, sb = median_pair(lambda: loop(ws), lambda: m.batch(ws))
        rows.append({"audios": n, "seconds": sec, "samples": sum(int(w.numel()) for w in ws), "passes": passes,
                     "loop_ms": round(tl, 3), "batch_ms": round(tb, 3), "loop_spread_ms": round(sl, 3),
                     "batch_spread_ms": round(sb, 3), "speedup": round(tl / tb, 2), "max_abs_batch_vs_loop": round(diff, 5)})
        del ws, out, ref

sweep = []
ws = audios(max(args.counts), max(args.seconds))
for ms in args.sweep:
    p0 = m.passes
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    m.batch(ws, max_samples=ms)
    passes = m.passes - p0
    peak = torch.cuda.max_memory_allocated() - base
    ta, tb, _, sb = median_pair(lambda: m.batch(ws, max_samples=ms), lambda: m.batch(ws, max_samples=ms))
    sweep.append({"max_samples": ms, "passes": passes, "batch_ms": round(min(ta, tb), 3), "spread_ms": round(sb, 3),
                  "peak_workspace_mb": round(peak / 2 ** 20, 1)})
slot_samples = sum((int(w.numel()) + 319) // 320 * 320 for w in ws)
del ws

# the segmented GroupNorm alone on conv 0's output of a full default pass: 32 equal segments, device time by events
plan = m.pack_plan([m.MAX_SAMPLES // 32 - 320] * 32)
R0, CH = plan["rows0"], 512
x = (torch.randn(R0, CH, device=DEV) * 0.5).half()
y = torch.empty_like(x)
gamma, beta = torch.ones(CH, device=DEV), torch.zeros(CH, device=DEV)
scratch = torch.empty(2 * CH * (sum((t + 255) // 256 for t in plan["cn_len"]) + 32), dtype=torch.float32, device=DEV)
starts, lens = (C.c_int32 * 32)(*plan["cn_start"]), (C.c_int32 * 32)(*plan["cn_len"])


def cnorm():
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().gsv_op_channel_norm_seg(x.data_ptr(), R0, CH, 32, starts, lens, gamma.data_ptr(), beta.data_ptr(), 1e-5, 7,
                                                  scratch.data_ptr(), y.data_ptr(), _lib.GSV_F16, st), "gsv_op_channel_norm_seg")


for _ in range(3):
    cnorm()
ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
for a, b in ev:
    a.record(); cnorm(); b.record()
torch.cuda.synchronize()
cn_ms = statistics.median(a.elapsed_time(b) for a, b in ev)
cn_bytes = 3 * R0 * CH * 2
kernel_a = {"rows": R0, "channels": CH, "segments": 32, "bytes": cn_bytes, "ms": round(cn_ms, 4),
            "tb_per_s": round(cn_bytes / cn_ms / 1e9, 2), "floor_ms_at_6.3_tb_per_s": round(cn_bytes / 6.3e9, 4)}
del x, y, scratch

pipeline = None
if args.voices > 0:
    from gsv.TTS_infer_pack.TTS import TTS
    tts = TTS({"device": DEV, "is_half": True, "version": "v2", "max_batch": 4, "max_seq": 600})
    tts.init_t2s_weights(state={"weight": S.make_t2s_state_dict(S.T2S_V2_CONFIG, seed=0, suppress_eos=True), "config": S.T2S_V2_CONFIG})
    tts.init_vits_weights(state={"weight": S.make_vits_state_dict(S.VITS_V2_CONFIG, seed=0), "config": dict(S.VITS_V2_CONFIG)})
    tts.init_cnhuhbert_weights(state_dict=hubert_sd)
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

        def together():
            fresh()
            return tts.make_voices(specs)

        def host_only():
            return [tts._prompt_wav16k(sp["ref_audio_path"]) for sp in specs]

        pm = tts.cnhuhbert_model.model
        p0 = pm.passes
        together()
        passes = pm.passes - p0
        t1, tm, s1, sm = median_pair(one_by_one, together)
        th, _, sh, _ = median_pair(host_only, host_only)
        pipeline = {"voices": args.voices, "seconds": 6, "passes": passes, "make_voice_x_n_ms": round(t1, 3), "make_voices_ms": round(tm, 3),
                    "make_voice_spread_ms": round(s1, 3), "make_voices_spread_ms": round(sm, 3),
                    "host_load_resample_ms": round(th, 3), "host_spread_ms": round(sh, 3),
                    "make_voice_rest_ms": round(t1 - th, 3), "make_voices_rest_ms": round(tm - th, 3),
                    "speedup": round(t1 / tm, 2)}

print(json.dumps({"tool": "voice_enrol_bench", "device": torch.cuda.get_device_name(0), "default_max_samples": m.MAX_SAMPLES,
                  "reps": args.reps, "rows": rows,
                  "sweep": {"audios": max(args.counts), "seconds": max(args.seconds), "slot_samples": slot_samples, "points": sweep},
                  "kernel_a": kernel_a, "pipeline": pipeline}))
