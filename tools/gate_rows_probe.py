"""One gated GEMM of the DiT (out-projection K = 1024 or FF2 K = 2048, 1024 outputs, fp16, residual) with ONE gate vector (the
default kernels) against per-row gates (gate_rows = 934: the GROWS instantiations of csrc/gemm_sk.hip / gemm_lds.hip), at the
row counts of 1 .. 32 live 934-frame rows.  HIP-event time per launch, medians of --reps launches after 10 warm-up launches, the
two forms alternating.  Prints one JSON line per shape with the route each form took.

    python tools/gate_rows_probe.py [--reps 50] [--rows 1,2,3,4,5,8,16,32]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gpt-sovits_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rows", default="1,2,3,4,5,8,16,32")
    a = ap.parse_args()
    from _conv_routes import decode_route
    from gsv import _lib
    _lib.init(0)
    lib, dev, T, Cout = _lib.lib(), "cuda:0", 934, 1024
    for B in [int(x) for x in a.rows.split(",")]:
        for K in (1024, 2048):
            R = B * T
            x = torch.randn(R, K, device=dev).half()
            w = (torch.randn(Cout, K, device=dev) / K ** 0.5).half()
            bias, gate = torch.randn(Cout, device=dev), torch.randn(B, Cout, device=dev)
            res, y = torch.randn(R, Cout, device=dev).half(), torch.empty(R, Cout, device=dev).half()
            d = _lib.ConvDesc()
            d.x, d.w, d.bias, d.y, d.res, d.gate = x.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), res.data_ptr(), gate.data_ptr()
            d.T_in = d.T_out = R
            d.Cin, d.Cout, d.taps, d.stride, d.dil, d.pad, d.scale, d.Z, d.res_dtype = K, Cout, 1, 1, 1, 0, 1.0, 1, 2
            ms, route = {"one": [], "rows": []}, {}
            for it in range(a.reps + 10):
                for form, gr in (("one", 0), ("rows", T)):
                    d.gate_rows, d.gate_ld = gr, Cout if gr else 0
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    _lib.check(lib.gsv_op_conv1d(C.byref(d), _lib.GSV_F16, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "conv1d")
                    e1.record()
                    route[form] = decode_route(int(lib.gsv_debug_last_conv_route(1)))
                    torch.cuda.synchronize()
                    if it >= 10:
                        ms[form].append(e0.elapsed_time(e1) * 1e3)
            one, rows = statistics.median(ms["one"]), statistics.median(ms["rows"])
            print(json.dumps({"live_rows": B, "R": R, "K": K, "route": route["one"], "us_one_gate": round(one, 2), "us_per_row_gates": round(rows, 2),
                              "ratio": round(rows / one, 4), "min_max_one": [round(min(ms["one"]), 2), round(max(ms["one"]), 2)],
                              "min_max_rows": [round(min(ms["rows"]), 2), round(max(ms["rows"]), 2)]}), flush=True)


if __name__ == "__main__":
    main()
