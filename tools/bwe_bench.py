"""Times AP-BWE super-sampling (csrc/bwe.hip through gsv.tools.audio_sr.AP_BWE) at the assumed published 24k -> 48k shape
(n_fft 1024, hop 80, win 320, 512 channels x 8 ConvNeXt layers per branch) on 10 s and 60 s of 24 kHz input, fp16 and fp32.
Prints one JSON line: ms per call, output-audio seconds per second, algorithmic FLOP and bytes per call (from the shapes),
and the share of the matching MFMA peak (fp16 2.5 PFLOP/s dense, fp32 157 TFLOP/s; HBM 8 TB/s) under whichever bound
applies.  --cpu-baseline times the torch-on-CPU restatement of the same computation (torch.stft / istft, the two-branch
model in torch.nn.functional) with at most 16 threads."""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpt-sovits_amd"))
import torch  # noqa: E402

from gsv import synthetic as S  # noqa: E402

PEAK = {"f16": 2.5e15, "f32": 157.3e12}
HBM = 8.0e12


def counts(cfg, n_in, orig=24000, es=2):
    """(flop, bytes) of one call: DFT / iDFT GEMMs (fp32), conv_pre, 2 GEMMs per block per branch, post head; bytes =
    weights once + the activations each launch reads and writes"""
    F, hop, C, L = cfg["n_fft"], cfg["hop_size"], cfg["ConvNeXt_channels"], cfg["ConvNeXt_layers"]
    B = F // 2 + 1
    n_new = math.ceil(n_in * cfg["hr_sampling_rate"] / orig)
    T = 1 + n_new // hop
    fl_dft = 2 * T * F * 2 * B * 2
    fl_model = 2 * (2 * T * B * 7 * C) + L * 2 * (2 * 2 * T * C * 3 * C) + 2 * T * C * 3 * B
    w = 2 * (7 * B * C + L * 6 * C * C) * es + 3 * B * C * es + 2 * 2 * B * F * 4
    act = (T * F * 4 * 2 + T * 2 * B * 4 * 4 + 2 * T * B * es            # frames, re|im, conv_pre operand
           + 2 * T * C * es * 3                                          # conv_pre + norm
           + L * 24 * T * C * es                                         # per layer: mix (2 -> 4), GEMM1 (2 -> 6), GEMM2 (6 + 2 -> 2)
           + 2 * T * C * es * 2 + T * 3 * B * 4 * 2 + T * 2 * B * 4 * 2  # post norm, post GEMMs, spectrum
           + T * F * 4 + n_new * 4)                                      # iDFT frames, OLA output
    return fl_dft + fl_model, fl_dft, w + act, T, n_new


def cpu_restatement(sd, cfg, x, orig):
    """torch CPU: the reference's computation restated with torch.nn.functional (no reference code)"""
    from gsv.tools.audio_sr import resample
    F_, hop, win, L = cfg["n_fft"], cfg["hop_size"], cfg["win_size"], cfg["ConvNeXt_layers"]
    f = torch.nn.functional
    y = resample(x, orig, cfg["hr_sampling_rate"])
    w = torch.hann_window(win)
    X = torch.stft(y, F_, hop, win, window=w, center=True, pad_mode="reflect", return_complex=True)
    la, ph = torch.log(X.abs() + 1e-4), torch.angle(X)

    def ln(t, p):
        return f.layer_norm(t.transpose(1, 2), (t.shape[1],), sd[p + ".weight"], sd[p + ".bias"], 1e-6).transpose(1, 2)

    xm = ln(f.conv1d(la, sd["conv_pre_mag.weight"], sd["conv_pre_mag.bias"], padding=3), "norm_pre_mag")
    xp = ln(f.conv1d(ph, sd["conv_pre_pha.weight"], sd["conv_pre_pha.bias"], padding=3), "norm_pre_pha")

    def block(t, p):
        h = f.conv1d(t, sd[p + "dwconv.weight"], sd[p + "dwconv.bias"], padding=3, groups=t.shape[1]).transpose(1, 2)
        h = f.layer_norm(h, (h.shape[-1],), sd[p + "norm.weight"], sd[p + "norm.bias"], 1e-6)
        h = f.linear(f.gelu(f.linear(h, sd[p + "pwconv1.weight"], sd[p + "pwconv1.bias"])), sd[p + "pwconv2.weight"], sd[p + "pwconv2.bias"])
        return t + (sd[p + "gamma"] * h).transpose(1, 2)

    for i in range(L):
        xm = xm + xp
        xp = xp + xm
        xm, xp = block(xm, f"convnext_mag.{i}."), block(xp, f"convnext_pha.{i}.")
    xm, xp = ln(xm, "norm_post_mag").transpose(1, 2), ln(xp, "norm_post_pha").transpose(1, 2)
    mag = la + f.linear(xm, sd["linear_post_mag.weight"], sd["linear_post_mag.bias"]).transpose(1, 2)
    pha = torch.atan2(f.linear(xp, sd["linear_post_pha_i.weight"], sd["linear_post_pha_i.bias"]),
                      f.linear(xp, sd["linear_post_pha_r.weight"], sd["linear_post_pha_r.bias"])).transpose(1, 2)
    a = torch.exp(mag)
    return torch.istft(torch.complex(a * torch.cos(pha), a * torch.sin(pha)), F_, hop, win, window=w, center=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, nargs="+", default=[10.0, 60.0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-baseline", action="store_true")
    a = ap.parse_args()
    cfg = dict(S.BWE_24K_48K_CONFIG)
    sd = S.make_bwe_state_dict(cfg, 0)
    res = {"what": "ap_bwe_24k_48k", "config": cfg, "runs": []}
    if a.cpu_baseline:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        for sec in a.seconds:
            x = S.hash_symmetric("bwe_bench_in", (int(24000 * sec),), 0.5, 1).view(1, -1)
            with torch.no_grad():
                t0 = time.perf_counter()
                y = cpu_restatement(sd, cfg, x, 24000)
                dt = time.perf_counter() - t0
            res["runs"].append({"device": "cpu", "threads": torch.get_num_threads(), "seconds_in": sec, "ms_per_call": dt * 1e3,
                                "audio_s_per_s": y.shape[-1] / 48000 / dt})
        print(json.dumps(res))
        return
    from gsv.tools.audio_sr import AP_BWE
    for dt_name, dtype in (("f16", torch.float16), ("f32", torch.float32)):
        m = AP_BWE("cuda:0", state={"generator": sd}, config=cfg, dtype=dtype)
        for sec in a.seconds:
            n = int(24000 * sec)
            x = S.hash_symmetric("bwe_bench_in", (n,), 0.5, 1).view(1, -1).cuda()
            out = m.forward_device(x, 24000)
            torch.cuda.synchronize()
            times = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                out = m.forward_device(x, 24000)
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
            best = min(times)
            fl, fl_dft, by, T, n_new = counts(cfg, n, es=2 if dtype == torch.float16 else 4)
            # DFT GEMMs run in fp32 in both modes: their time at the fp32 peak, the model's at the engine dtype's
            t_compute = fl_dft / PEAK["f32"] + (fl - fl_dft) / PEAK[dt_name]
            t_mem = by / HBM
            bound = "compute" if t_compute >= t_mem else "memory"
            res["runs"].append({"dtype": dt_name, "seconds_in": sec, "frames": T, "ms_per_call": best * 1e3,
                                "ms_median": sorted(times)[len(times) // 2] * 1e3, "audio_s_per_s": out.shape[0] / 48000 / best,
                                "gflop": fl / 1e9, "gflop_dft_fp32": fl_dft / 1e9, "mbytes": by / 1e6, "bound": bound,
                                "share_of_bound": max(t_compute, t_mem) / best, "tflops": fl / best / 1e12,
                                "finite": bool(torch.isfinite(out).all())})
        del m
    print(json.dumps(res))


if __name__ == "__main__":
    main()
