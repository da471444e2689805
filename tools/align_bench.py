"""What the phoneme alignment costs: SynthesizerTrn.decode_segments of 32 sentences x 4 s (100 codes =
200 frames each, 40..80 phonemes) on the full-size v2 model with synthetic weights, with and without one span per sentence, and
the two alignment launches alone on operands of the same shape.  Medians of 7 in one process, after 2 warm-up rounds; the two
arms alternate.  Prints one JSON line.

    python tools/align_bench.py [--dtype fp16|fp32] [--sentences 32] [--rounds 7]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gpt-sovits_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "fp32"])
    ap.add_argument("--sentences", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import numpy as np
    import torch
    from gsv import _lib
    from gsv import synthetic as S
    from gsv.module.models import SynthesizerTrn

    dev, dtype = "cuda:0", torch.float16 if a.dtype == "fp16" else torch.float32
    cfg = S.VITS_V2_CONFIG
    d, mk = cfg["data"], dict(cfg["model"])
    version = mk.pop("version", "v2")
    m = SynthesizerTrn(d["filter_length"] // 2 + 1, cfg["train"]["segment_size"] // d["hop_length"], n_speakers=d["n_speakers"],
                       version=version, device=dev, dtype=dtype, n_symbols=cfg["n_symbols"], **mk)
    m.load_state_dict(S.make_vits_state_dict(cfg, seed=3))
    n, T = a.sentences, 100
    L = [40 + (40 * i) // max(n - 1, 1) for i in range(n)]
    codes = [torch.from_numpy(S.hash_ints(f"ab_codes{i}", T, 1024, 5)).view(1, 1, -1).to(dev) for i in range(n)]
    text = [torch.from_numpy(S.hash_ints(f"ab_text{i}", L[i], cfg["n_symbols"], 5)).view(1, -1).to(dev) for i in range(n)]
    refer = torch.from_numpy(S.hash_uniform("ab_refer", 1025 * 37, 11).reshape(1, 1025, 37).copy()).to(dev)
    voices, seeds = [(refer, None)] * n, list(range(n))

    def decode(align):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.decode_segments(codes, text, voices, seeds, align=align)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    spans = [True] * n
    for _ in range(2):
        decode(None), decode(spans)
    plain, marked = [], []
    for _ in range(a.rounds):
        plain.append(decode(None))
        marked.append(decode(spans))
    scores = [s for _, s in m.last_alignment]

    # the two launches alone, on random operands of the engine's shape (q [.][512], k|v [.][1024])
    l = _lib.lib()
    tab = np.zeros(n, np.dtype(_lib.ALIGN_SPAN_DTYPE))
    f = p = o = 0
    for i in range(n):
        tab[i] = (f, 2 * T, p, L[i], o, 0)
        f, p, o = f + 2 * T, p + L[i], o + L[i]
    nbytes = l.gsv_op_align_workspace(n, tab.ctypes.data_as(C.POINTER(_lib.AlignSpan)), None)
    g = torch.Generator().manual_seed(0)
    q = (3 * torch.randn(f, 512, generator=g)).to(dtype).to(dev)
    k = torch.randn(p, 1024, generator=g).to(dtype).to(dev)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    dtab = torch.from_numpy(tab.view(np.int32).reshape(n, 6).copy()).to(dev)
    ends = torch.empty(o, dtype=torch.int32, device=dev)
    score = torch.empty(n, dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream()
    sp = C.c_void_p(st.cuda_stream)
    logp = lambda: _lib.check(l.gsv_op_align_logp(q.data_ptr(), 512, k.data_ptr(), 1024, _lib.dtype_code(dtype), 4, 128, 128 ** -0.5,
                                                  dtab.data_ptr(), n, ws.data_ptr(), nbytes, sp))
    path = lambda: _lib.check(l.gsv_op_align_path(dtab.data_ptr(), n, ws.data_ptr(), nbytes, ends.data_ptr(), score.data_ptr(), sp))

    def timed(fn, reps=20):
        fn()
        out = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(reps):
                fn()
            e1.record(st)
            e1.synchronize()
            out.append(e0.elapsed_time(e1) / reps * 1e3)
        return out

    t_logp, t_path = timed(logp), timed(path)
    med = statistics.median
    print(json.dumps({
        "dtype": a.dtype, "sentences": n, "frames": 2 * T, "phonemes": [min(L), max(L)], "rounds": a.rounds,
        "decode_segments_ms": {"median": round(med(plain), 3), "min": round(min(plain), 3), "max": round(max(plain), 3)},
        "decode_segments_align_ms": {"median": round(med(marked), 3), "min": round(min(marked), 3), "max": round(max(marked), 3)},
        "align_logp_us": {"median": round(med(t_logp), 2), "min": round(min(t_logp), 2), "max": round(max(t_logp), 2)},
        "align_path_us": {"median": round(med(t_path), 2), "min": round(min(t_path), 2), "max": round(max(t_path), 2)},
        "mean_confidence": round(float(np.mean(scores)), 4)}))


if __name__ == "__main__":
    main()
