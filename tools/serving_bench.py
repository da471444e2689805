"""Open-arrival serving: the same seeded Poisson arrival trace, replayed in wall time, through three servers in ONE process
(full-size synthetic v2 weights, fp16, --voices enrolled voices, requests of 1-4 sentences x 4 s):

  (A) run() per request in arrival order -- what `wire.create_app` did before gsv.serving;
  (B) windowed batching: collect for W ms from the first waiting request, then run_batch with the shared flags (W swept);
  (C) gsv.serving.Server (chunk, admit_min, wave_hold swept).

The offered loads are fractions of the closed-batch throughput that this process measures first with
run_batch(all requests, shared_sovits=True).  Per server, setting and load: p50 / p95 of the time from submit to result,
delivered audio-seconds per second, and for (C) the mean slot occupancy and the waveform passes per second -- medians over
--repeats replays.  One JSON line per (server, setting, load), then a summary line.

    python tools/serving_bench.py [--requests 96] [--voices 32] [--slots 32] [--loads 0.3,0.6,0.9] [--windows-ms 10,40]
                                  [--chunks 8,32] [--admit-mins 1,8] [--wave-holds 0,2] [--repeats 7]

--version v3 | v4: the full-size synthetic v3 / v4 pipeline instead (DiT 1024 x 22, BigVGAN-v2 / the v4 HiFi-GAN), every voice with
its own prompt mel, --sample-steps (comma list, dealt round-robin to the requests).  The closed batch and (B) are
run_batch(shared_cfm=True), (A) is left out, (C) is Server() with the settings above -- the waveform stage as closed
_shared_cfm_stage passes -- and (D) is Server(continuous_cfm=True) for every --cfm-chunks x --cfm-rows at the first (C) setting:
the waveform stage as an open flow-matching session.  --handoff prints, before the replays, the device time of
CFMSession.fetch_mel for 1 / 8 / 32 finished rows of T_chunk frames against the per-slot fetch + slice + denorm_spec + cat it
replaces, next to the byte floor 2 * rows * (T - Tp) * 100 * 4 B.

    python tools/serving_bench.py --version v3 --sample-steps 8,16,32 [--cfm-chunks 1,2,4,8] [--cfm-rows 16,32,64] [--handoff]

--streaming: instead of the sweep, the same replay with --stream-share of the requests streaming (`return_fragment`, sent with
`Server.submit_stream`), through Server() at the first (C) setting -- streaming requests inside the sessions -- against the
scheduler as it was before: the same class with every streaming request exclusive (sessions drained and closed, run() alone,
all fragments at the end; `_ExclusiveStreams`).  Both in this process, --repeats alternating pairs over the same arrival
traces (the order within a pair flips from pair to pair).  Per load: submit-to-first-fragment and submit-to-last-fragment
p50 / p95 of the streaming requests, p50 / p95 of the others, audio-s/s -- medians over the pairs with the min..max spread of
the p50s -- and the same pairs with no streaming request at all (the two must not separate beyond that spread).
--postprocess prints first the cost of one gsv_postprocess_groups call for 32 fragments x 4 s against 32 gsv_postprocess
calls (device time between events, and wall time through the pipeline's methods with the copy to the host) next to the byte
floor (each sample read twice, written once).

--mixed-limits: instead of the sweep, the same replay with --odd-share of the requests drawn from the four kinds that are
exclusive without Scheduler(mixed_limits=True) (prompt-free, parallel_infer=False, best_of=2, arena-short), served with the
keyword and without it in alternating pairs: submit-to-result p50 / p95 of the odd and of the plain requests, audio-s/s.

    python tools/serving_bench.py --streaming [--stream-share 0.25] [--loads 0.3,0.6,0.9] [--postprocess]
    python tools/serving_bench.py --mixed-limits [--odd-share 0.1] [--loads 0.3,0.6,0.9]
"""
import argparse
import json
import os
import queue
import random
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gpt-sovits_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def _pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))] if xs else float("nan")


def _replay(arrivals, submit):
    """calls submit(i) at arrivals[i] seconds after the start; returns the start time"""
    t0 = time.perf_counter()
    for i, at in enumerate(arrivals):
        wait = t0 + at - time.perf_counter()
        if wait > 0:
            time.sleep(wait)
        submit(i)
    return t0


def _report(t0, arrivals, done_at, audio_s):
    lat = [done_at[i] - (t0 + arrivals[i]) for i in range(len(arrivals))]
    span = max(done_at) - t0
    return dict(p50_ms=round(1e3 * _pct(lat, 0.5), 1), p95_ms=round(1e3 * _pct(lat, 0.95), 1),
                audio_s_per_s=round(sum(audio_s) / span, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--requests", type=int, default=96)
    ap.add_argument("--voices", type=int, default=32)
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=100, help="AR tokens per sentence (25 tokens = 1 s)")
    ap.add_argument("--loads", default="0.3,0.6,0.9")
    ap.add_argument("--windows-ms", default="10,40")
    ap.add_argument("--chunks", default="8,32")
    ap.add_argument("--admit-mins", default="1,8")
    ap.add_argument("--wave-holds", default="0,2")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--version", default="v2", choices=["v2", "v3", "v4"])
    ap.add_argument("--sample-steps", default="32", help="v3 / v4: comma list, dealt round-robin to the requests")
    ap.add_argument("--cfm-chunks", default="1,2,4,8")
    ap.add_argument("--cfm-rows", default="16,32,64")
    ap.add_argument("--handoff", action="store_true", help="v3 / v4: time fetch_mel against the per-slot hand-off first")
    ap.add_argument("--streaming", action="store_true", help="streaming requests in the sessions against the exclusive path")
    ap.add_argument("--stream-share", type=float, default=0.25)
    ap.add_argument("--mixed-limits", action="store_true",
                    help="a share of prompt-free / naive / best_of / arena-short requests: Scheduler(mixed_limits=True) against without")
    ap.add_argument("--odd-share", type=float, default=0.1)
    ap.add_argument("--postprocess", action="store_true", help="time gsv_postprocess_groups against per-fragment gsv_postprocess first")
    a = ap.parse_args()
    from bench import build_tts, make_segments
    from gsv import synthetic as S
    dev = torch.device("cuda:0")
    N, TOK = a.requests, a.tokens
    v3 = a.version != "v2"
    shared = dict(shared_cfm=True) if v3 else dict(shared_sovits=True)
    if v3:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        from multivoice_v3_bench import build_v3
        tts = build_v3(dev, TOK, a.slots)
        if a.version == "v4":
            tts.configs.version = "v4"
            tts.init_vocoder("v4", state={"weight": S.make_vocoder_state_dict(dict(S.HIFIGAN_V4_CONFIG), seed=4),
                                          "config": dict(S.HIFIGAN_V4_CONFIG)})
        if a.handoff:
            handoff(tts, dev)
    else:
        tts = build_tts(dev, TOK, a.slots, dtype_half=True)
        tts.configs.max_seq = 80 + 160 + TOK + 16          # room for the longest voice's prompt
        tts.t2s_model = None
        tts.init_t2s_weights(tts.configs.t2s_weights_path, state=tts._t2s_state)
    if a.postprocess:
        postprocess_cost(tts, dev)
    rng = random.Random(a.seed)
    counts = [rng.randint(1, 4) for _ in range(N)]
    utt, segs = make_segments(sum(counts))
    n_ph = len(utt["prompt_phones"])
    mel_kw = (lambda i: dict(ref_mel=S.hash_symmetric(f"sv_mel{i}", (1, 100, 200 + (i * 53) % 400), 5.0, 3) - 5.0)) if v3 else (lambda i: {})
    voices = [tts.make_voice(torch.from_numpy(S.hash_ints(f"sv_sem{i}", 60 + (i * 37) % 100, 1024, 1)),
                             [S.make_refer_spec(frames=150 + 7 * i, seed=100 + i).to(dev).half()],
                             phones=S.hash_ints(f"sv_ph{i}", n_ph, 732, 1).tolist(), bert_features=torch.zeros(1024, n_ph),
                             norm_text="x" * n_ph, **mel_kw(i)) for i in range(a.voices)]
    params = dict(top_k=15, top_p=1.0, temperature=1.0, repetition_penalty=1.35, fragment_interval=0.01)
    reqs, at = [], 0
    for i, c in enumerate(counts):
        reqs.append(dict(params, segments=segs[at:at + c], batch_size=c, seed=7 + i, voice=voices[i % a.voices]))
        if v3:
            steps = [int(x) for x in a.sample_steps.split(",") if x]
            reqs[-1]["sample_steps"] = steps[i % len(steps)]
        at += c

    def alone(r):
        v = r["voice"]
        tts.set_prompt_cache(v["prompt_semantic"], [s for s, _ in v["refer_spec"]], phones=v["phones"],
                             bert_features=v["bert_features"], norm_text=v["norm_text"])
        return list(tts.run({k: x for k, x in r.items() if k != "voice"}))[0]

    # closed-batch capacity: everything at once through the shared stages (second of two passes: the first warms up)
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = tts.run_batch(reqs, **shared)
        torch.cuda.synchronize()
        closed_s = time.perf_counter() - t0
    audio_s = [w.shape[0] / sr for sr, w in outs]
    capacity = sum(audio_s) / closed_s
    if not v3:
        alone(reqs[0])
    print(json.dumps(dict(record="closed_batch", version=a.version, requests=N, sentences=sum(counts), audio_s=round(sum(audio_s), 1),
                          seconds=round(closed_s, 4), audio_s_per_s=round(capacity, 1))), flush=True)

    def trace(load, rep):
        r_ = random.Random(1000 * a.seed + rep)
        rate = load * capacity / (sum(audio_s) / N)       # requests per second
        t, out = 0.0, []
        for _ in range(N):
            t += r_.expovariate(rate)
            out.append(t)
        return out

    def serve_a(arrivals):
        q, done_at = queue.Queue(), [0.0] * N

        def worker():
            for _ in range(N):
                i = q.get()
                alone(reqs[i])
                done_at[i] = time.perf_counter()
        th = threading.Thread(target=worker)
        th.start()
        t0 = _replay(arrivals, q.put)
        th.join()
        return _report(t0, arrivals, done_at, audio_s)

    def serve_b(arrivals, window):
        q, done_at = queue.Queue(), [0.0] * N

        def worker():
            left = N
            while left:
                batch = [q.get()]
                end = time.perf_counter() + window
                while True:
                    try:
                        batch.append(q.get(timeout=max(0.0, end - time.perf_counter())))
                    except queue.Empty:
                        break
                tts.run_batch([reqs[i] for i in batch], **shared)
                now = time.perf_counter()
                for i in batch:
                    done_at[i] = now
                left -= len(batch)
        th = threading.Thread(target=worker)
        th.start()
        t0 = _replay(arrivals, q.put)
        th.join()
        return _report(t0, arrivals, done_at, audio_s)

    def serve_c(arrivals, **kw):
        done_at, futs = [0.0] * N, [None] * N
        server = tts.serve(slots=a.slots, **kw)

        def submit(i):
            futs[i] = server.submit(reqs[i])
            futs[i].add_done_callback(lambda f, i=i: done_at.__setitem__(i, time.perf_counter()))
        t0 = _replay(arrivals, submit)
        for f in futs:
            f.result()
        server.shutdown()
        st = server.scheduler.stats
        out = _report(t0, arrivals, done_at, audio_s)
        span = max(done_at) - t0
        out.update(occupancy=round(statistics.mean(st["occupancy"]) / a.slots, 3) if st["occupancy"] else 0.0,
                   waves_per_s=round(st["waves"] / span, 1), advances=st["advances"], admissions=st["admissions"],
                   sessions=st["sessions"])
        if kw.get("continuous_cfm"):
            out.update(cfm_live_dit_rows=round(statistics.mean(st["cfm_occupancy"]), 2) if st["cfm_occupancy"] else 0.0,
                       cfm_euler_steps=st["cfm_steps"], cfm_admissions=st["cfm_admissions"], vocoder_calls=st["vocoder_calls"])
        return out

    if a.mixed_limits:
        kw = dict(chunk=int(a.chunks.split(",")[0]), admit_min=int(a.admit_mins.split(",")[0]), wave_hold=int(a.wave_holds.split(",")[0]))
        vfree = tts.make_voice(torch.from_numpy(S.hash_ints("sv_sem_free", 60, 1024, 1)),
                               [S.make_refer_spec(frames=150, seed=99).to(dev).half()])
        mixed_limits_pairs(a, tts, reqs, audio_s, trace, kw, vfree)
        print(json.dumps(dict(record="engine", fallbacks=tts.t2s_model.engine_stats()[1])), flush=True)
        return
    if a.streaming:
        kw = dict(chunk=int(a.chunks.split(",")[0]), admit_min=int(a.admit_mins.split(",")[0]), wave_hold=int(a.wave_holds.split(",")[0]))
        if v3:
            kw.update(continuous_cfm=True, cfm_chunk=int(a.cfm_chunks.split(",")[0]), cfm_rows=int(a.cfm_rows.split(",")[0]))
        streaming_pairs(a, tts, reqs, audio_s, trace, kw)
        print(json.dumps(dict(record="engine", fallbacks=tts.t2s_model.engine_stats()[1])), flush=True)
        return
    settings = [] if v3 else [("A", "run() per request", serve_a, {})]
    settings += [("B", f"window {w} ms", serve_b, dict(window=float(w) / 1e3)) for w in a.windows_ms.split(",") if w]
    settings += [("C", f"chunk {c} admit_min {m} wave_hold {h}", serve_c, dict(chunk=int(c), admit_min=int(m), wave_hold=int(h)))
                 for c in a.chunks.split(",") if c for m in a.admit_mins.split(",") if m for h in a.wave_holds.split(",") if h]
    if v3:
        first = dict(next((kw for kind, _, _, kw in settings if kind == "C"), {}))
        settings += [("D", f"continuous_cfm cfm_chunk {k} cfm_rows {r} ({' '.join(f'{x} {y}' for x, y in first.items())})", serve_c,
                      dict(first, continuous_cfm=True, cfm_chunk=int(k), cfm_rows=int(r)))
                     for k in a.cfm_chunks.split(",") if k for r in a.cfm_rows.split(",") if r]
    for load in [float(x) for x in a.loads.split(",") if x]:
        for kind, name, fn, kw in settings:
            runs = [fn(trace(load, rep), **kw) for rep in range(a.repeats)]
            med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
            print(json.dumps(dict(record="serve", server=kind, setting=name, load=load, repeats=a.repeats, **med)), flush=True)
    print(json.dumps(dict(record="engine", fallbacks=tts.t2s_model.engine_stats()[1])), flush=True)


def mixed_limits_pairs(a, tts, reqs, audio_s, trace, kw, vfree):
    """--mixed-limits: the Poisson replay with --odd-share of the requests drawn from the four kinds that are exclusive without
    Scheduler(mixed_limits=True) -- prompt-free, parallel_infer=False, best_of=2, a sentence short of arena room -- served by
    that scheduler and by the same class without the keyword: same process, alternating pairs, medians of --repeats, per load.
    Reported separately for the odd and the plain requests of the mix: submit-to-result p50 / p95; and audio-s/s of the run
    (the audio seconds are those of each server's own results: an odd request's length is not the closed batch's)."""
    from gsv.serving import Scheduler, Server
    N = len(reqs)
    r_ = random.Random(99 + a.seed)
    odd = {i: n % 4 for n, i in enumerate(i for i in range(N) if r_.random() < a.odd_share)}   # the four kinds dealt in turn
    from gsv.TTS_infer_pack.TTS import early_stop_num
    budget = min(1500, int(early_stop_num(tts.configs)) + 1)
    rq = []
    for i, r in enumerate(reqs):
        kind = odd.get(i)
        if kind == 0:
            r = dict(r, voice=vfree)
        elif kind == 1:
            r = dict(r, parallel_infer=False)
        elif kind == 2:
            r = dict(r, best_of=2)
        elif kind == 3:          # several sentences' phones in one, until text + prompt leave the arena less than the full budget
            fixed = len(r["voice"]["phones"]) + int(r["voice"]["prompt_semantic"].numel()) + 2
            parts, k = [r["segments"][0]], 1
            room = lambda ps: tts.t2s_model.max_seq - fixed - sum(len(p_["phones"]) for p_ in ps)
            while room(parts) >= budget:
                parts.append(reqs[(i + k) % N]["segments"][0])
                k += 1
            if room(parts) < 1:
                raise SystemExit(f"request {i}: {room(parts)} steps of room: no arena-short sentence can be built from these segments")
            long = dict(parts[0], phones=[x for p_ in parts for x in p_["phones"]], norm_text="".join(p_["norm_text"] for p_ in parts),
                        bert_features=torch.cat([p_["bert_features"] for p_ in parts], 1))
            r = dict(r, segments=[long] + list(r["segments"][1:]))
        rq.append(r)

    def serve(arrivals, mixed):
        done_at, futs, secs = [0.0] * N, [None] * N, [0.0] * N
        server = Server(Scheduler(tts, slots=a.slots, **kw, **(dict(mixed_limits=True) if mixed else {})))

        def submit(i):
            futs[i] = server.submit(rq[i])
            futs[i].add_done_callback(lambda f, i=i: done_at.__setitem__(i, time.perf_counter()))
        t0 = _replay(arrivals, submit)
        for i, f in enumerate(futs):
            sr, w = f.result()
            secs[i] = w.shape[0] / sr
        server.shutdown()
        st = server.scheduler.stats
        lat = lambda ids: [done_at[i] - (t0 + arrivals[i]) for i in ids]
        plain = [i for i in range(N) if i not in odd]
        ms = lambda xs, q: round(1e3 * _pct(xs, q), 1) if xs else None
        return dict(odd_p50_ms=ms(lat(sorted(odd)), 0.5), odd_p95_ms=ms(lat(sorted(odd)), 0.95),
                    plain_p50_ms=ms(lat(plain), 0.5), plain_p95_ms=ms(lat(plain), 0.95),
                    audio_s_per_s=round(sum(secs) / (max(done_at) - t0), 1), sessions=st["sessions"], exclusive=st["exclusive"])

    servers = (("mixed_limits", True), ("exclusive", False))
    for load in [float(x) for x in a.loads.split(",") if x]:
        runs = {name: [] for name, _ in servers}
        for rep_ in range(a.repeats):
            for name, mixed in (servers if rep_ % 2 == 0 else servers[::-1]):
                runs[name].append(serve(trace(load, rep_), mixed))
        for name, _ in servers:
            med = {k: (statistics.median(r[k] for r in runs[name]) if runs[name][0][k] is not None else None) for k in runs[name][0]}
            spread = {k: [min(r[k] for r in runs[name]), max(r[k] for r in runs[name])]
                      for k in ("odd_p50_ms", "plain_p50_ms", "audio_s_per_s") if runs[name][0][k] is not None}
            print(json.dumps(dict(record="mixed_limits", server=name, load=load, odd_share=a.odd_share, odd=len(odd),
                                  kinds=[sum(k == j for k in odd.values()) for j in range(4)], requests=N, pairs=a.repeats,
                                  setting=kw, **med, spread=spread)), flush=True)


def streaming_pairs(a, tts, reqs, audio_s, trace, kw):
    """--streaming (module docstring)"""
    from gsv.serving import Scheduler, Server
    N = len(reqs)

    class _ExclusiveStreams(Scheduler):
        """the scheduler before streaming requests were session citizens: each is a FIFO barrier served by run() alone"""
        def _session_rows(self, pl):
            return None if pl["opts"]["return_fragment"] else super()._session_rows(pl)

    def serve(arrivals, streams, cls, reqs):
        first_at, done_at, handles = [0.0] * N, [0.0] * N, [None] * N
        server = Server(cls(tts, slots=a.slots, **kw))
        readers = []

        def read(i, stream):
            for n, _ in enumerate(stream):
                if n == 0:
                    first_at[i] = time.perf_counter()
            done_at[i] = time.perf_counter()

        def submit(i):
            if i in streams:
                handles[i] = server.submit_stream(reqs[i])
                readers.append(threading.Thread(target=read, args=(i, handles[i])))
                readers[-1].start()
            else:
                handles[i] = server.submit(reqs[i])
                handles[i].add_done_callback(lambda f, i=i: done_at.__setitem__(i, time.perf_counter()))
        t0 = _replay(arrivals, submit)
        for i, h in enumerate(handles):
            (h.future if i in streams else h).result()
        for th in readers:
            th.join()
        server.shutdown()
        st = server.scheduler.stats
        lat = lambda at, ids: [at[i] - (t0 + arrivals[i]) for i in ids]
        plain = [i for i in range(N) if i not in streams]
        ss = sorted(streams)
        ms = lambda xs, q: round(1e3 * _pct(xs, q), 1) if xs else None
        return dict(first_p50_ms=ms(lat(first_at, ss), 0.5), first_p95_ms=ms(lat(first_at, ss), 0.95),
                    last_p50_ms=ms(lat(done_at, ss), 0.5), last_p95_ms=ms(lat(done_at, ss), 0.95),
                    plain_p50_ms=ms(lat(done_at, plain), 0.5), plain_p95_ms=ms(lat(done_at, plain), 0.95),
                    audio_s_per_s=round(sum(audio_s) / (max(done_at) - t0), 1), sessions=st["sessions"], exclusive=st["exclusive"])

    servers = (("sessions", Scheduler), ("exclusive", _ExclusiveStreams))
    for load in [float(x) for x in a.loads.split(",") if x]:
        for share in (a.stream_share, 0.0):
            r_ = random.Random(77 + a.seed)
            streams = {i for i in range(N) if r_.random() < share}
            # an interactive caller streams sentence by sentence: batch_size 1, one fragment per sentence, for both servers
            rq = [dict(r, batch_size=1) if i in streams else r for i, r in enumerate(reqs)]
            runs = {name: [] for name, _ in servers}
            for rep in range(a.repeats):
                for name, cls in (servers if rep % 2 == 0 else servers[::-1]):
                    runs[name].append(serve(trace(load, rep), streams, cls, rq))
            for name, _ in servers:
                med = {k: (statistics.median(r[k] for r in runs[name]) if runs[name][0][k] is not None else None) for k in runs[name][0]}
                spread = {k: [min(r[k] for r in runs[name]), max(r[k] for r in runs[name])]
                          for k in ("first_p50_ms", "last_p50_ms", "plain_p50_ms", "audio_s_per_s") if runs[name][0][k] is not None}
                print(json.dumps(dict(record="stream", server=name, load=load, stream_share=share, streams=len(streams), requests=N,
                                      pairs=a.repeats, setting=kw, **med, spread=spread)), flush=True)


def postprocess_cost(tts, dev):
    """--postprocess (module docstring): 32 fragments of 4 s at the pipeline's rate and precision"""
    import ctypes as C
    from gsv import _lib
    sr, n = int(tts.configs.sampling_rate), 32
    L = 4 * sr
    wav = (torch.rand(n * L + 8, device=dev) * 2.4 - 1.2).to(tts.precision)
    frags = [wav[3 + i * L:3 + (i + 1) * L] for i in range(n)]                 # views, not 16-byte aligned
    gap = int(sr * 0.3)
    code = _lib.GSV_F16 if tts.precision == torch.float16 else _lib.GSV_F32
    l, st = _lib.lib(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    lens = (C.c_int * n)(*[L] * n)
    ptrs = (C.c_void_p * n)(*[f.data_ptr() for f in frags])
    gn, gg, off = (C.c_int * n)(*[1] * n), (C.c_int * n)(*[gap] * n), (C.c_longlong * (n + 1))()
    need = int(l.gsv_postprocess_groups_workspace(lens, n))
    table, work = torch.empty(need, dtype=torch.uint8).pin_memory(), torch.empty(need, dtype=torch.uint8, device=dev)
    pcm = torch.empty(n * (L + gap), dtype=torch.int16, device=dev)
    one = [((C.c_void_p * 1)(f.data_ptr()), (C.c_int * 1)(L)) for f in frags]

    def grouped():
        _lib.check(l.gsv_postprocess_groups(ptrs, lens, n, code, gn, gg, n, pcm.data_ptr(), off, table.data_ptr(), work.data_ptr(), st), "groups")

    def single():
        for i, (p, k) in enumerate(one):
            _lib.check(l.gsv_postprocess(p, k, 1, code, gap, pcm.data_ptr() + 2 * i * (L + gap), st), "postprocess")
    dev_ms = {}
    for name, fn in (("groups_one_call", grouped), ("postprocess_32_calls", single)):
        ts = []
        for it in range(12):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= 2:
                ts.append(e0.elapsed_time(e1))
        dev_ms[name] = round(statistics.median(ts), 4)
    wall_ms = {}
    for name, fn in (("postprocess_fragments", lambda: tts.postprocess_fragments([([f], 0.3) for f in frags])),
                     ("audio_postprocess_x32", lambda: [tts.audio_postprocess([[f]], sr, None, 1.0, False, 0.3, False) for f in frags])):
        ts = []
        for it in range(9):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append(1e3 * (time.perf_counter() - t0))
        wall_ms[name] = round(statistics.median(ts[2:]), 4)
    esz = 2 if tts.precision == torch.float16 else 4
    floor = n * L * (2 * esz + 2) + n * gap * 2
    print(json.dumps(dict(record="postprocess", fragments=n, samples_each=L, dtype="f16" if esz == 2 else "f32", gap=gap,
                          device_ms=dev_ms, wall_ms_with_host_copy=wall_ms, floor_bytes=floor,
                          floor_us_at_6p3_TBps=round(floor / 6.3e12 * 1e6, 2))), flush=True)


def handoff(tts, dev):
    """device time of fetch_mel for 1 / 8 / 32 finished rows of T_chunk frames (Tp = 468) against the hand-off it replaces"""
    from gsv import synthetic as S
    from gsv.TTS_infer_pack.TTS import denorm_spec, spec_max, spec_min
    cfm, T, Tp = tts.vits_model.cfm, tts.vocoder_configs["T_chunk"], 468
    for B in (1, 8, 32):
        mu = S.hash_symmetric("ho_mu", (B, T, 512), 1.0, B).to(dev).half()
        pr = [S.hash_symmetric("ho_p", (1, 100, Tp), 1.0, b).to(dev).half() for b in range(B)]
        L = T - Tp
        out = torch.empty(100, B * L, dtype=torch.float32, device=dev)
        ms = {"fetch_mel": [], "per_slot": []}
        for it in range(8):
            for mode in ms:
                with cfm.open_session(B, T) as s:
                    slots = s.admit(mu, pr, 1, 0.0, seeds=list(range(1, B + 1)))
                    s.step(1)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    if mode == "fetch_mel":
                        s.fetch_mel(slots, [b * L for b in range(B)], out, spec_min, spec_max)
                    else:
                        pred = torch.stack([s.fetch(sl)[:, Tp:] for sl in slots])
                        denorm_spec(pred.permute(1, 0, 2).contiguous().view(100, -1).unsqueeze(0))
                    e1.record()
                    torch.cuda.synchronize()
                    if it:
                        ms[mode].append(e0.elapsed_time(e1))
        floor_bytes = 2 * B * L * 100 * 4
        print(json.dumps(dict(record="handoff", rows=B, T=T, Tp=Tp, fetch_mel_ms=round(statistics.median(ms["fetch_mel"]), 4),
                              per_slot_ms=round(statistics.median(ms["per_slot"]), 4), floor_bytes=floor_bytes,
                              floor_us_at_6p3_TBps=round(floor_bytes / 6.3e12 * 1e6, 3))), flush=True)


if __name__ == "__main__":
    main()
