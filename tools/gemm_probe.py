"""Times one Linear-shaped launch of gsv_op_conv1d (taps = 1) with HIP events over back-to-back launches; used to probe
the GEMM kernels (GSV_NO_GEMM_SK and the other switches of csrc/conv_launch.h select variants).  Not part of the product.

  gemm_probe.py [TxKxN ...]     the dispatcher's kernel for each shape (no bias, fp16 out)
  gemm_probe.py --panel         the prefill's four GEMMs (QKV, out-projection, FFN1, FFN2, with their epilogue forms) at
                                M = 180 * {8, 12, 16, 24, 32, 64, 128}: the dispatcher against every tile of the panel kernel
                                (csrc/gemm_panel.hip, gsv_op_gemm_panel); one JSON line per (shape, M)
"""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpt-sovits_amd"))
import torch  # noqa: E402

from gsv import _lib  # noqa: E402


def _time(launch, n=50):
    for _ in range(3):
        _lib.check(launch())
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def panel():
    l = _lib.lib()
    st = torch.cuda.current_stream()
    sp = C.c_void_p(st.cuda_stream)
    # name, K, N, out_f32, residual, post_act
    shapes = [("qkv", 512, 1536, 0, False, 0), ("out", 512, 512, 1, True, 0), ("ffn1", 512, 2048, 0, False, 1), ("ffn2", 2048, 512, 1, True, 0)]
    for name, K, N, out_f32, has_res, post in shapes:
        for rows in (8, 12, 16, 24, 32, 64, 128):
            M = 180 * rows
            x = torch.randn(M, K, device="cuda", dtype=torch.float16)
            w = torch.randn(N, K, device="cuda", dtype=torch.float16) / K ** 0.5
            b = torch.randn(N, device="cuda")
            res = torch.randn(M, N, device="cuda", dtype=torch.float16) if has_res else None
            y = torch.zeros(M, N, device="cuda", dtype=torch.float32 if out_f32 else torch.float16)
            d = _lib.ConvDesc(x=x.data_ptr(), w=w.data_ptr(), bias=b.data_ptr(), y=y.data_ptr(), res=res.data_ptr() if has_res else None,
                              T_in=M, T_out=M, Cin=K, Cout=N, taps=1, stride=1, dil=1, pad=0, post_act=post, scale=1.0,
                              out_f32=out_f32, res_dtype=2 if has_res else 0)
            row = {"gemm": name, "M": M, "K": K, "N": N}
            l.gsv_debug_last_conv_route(1)
            row["dispatcher_us"] = round(_time(lambda: l.gsv_op_conv1d(C.byref(d), 1, sp)), 2)
            row["dispatcher_route"] = hex(l.gsv_debug_last_conv_route(1))
            y_ref = y.clone()
            for tile in (1, 2, 3, 4):          # 4 = 96 x 128 with gemm_t64's summation: same bits as the dispatcher where that is gemm_t64
                y.zero_()
                row[f"tile{tile}_us"] = round(_time(lambda: l.gsv_op_gemm_panel(C.byref(d), 1, tile, sp)), 2)
                row[f"tile{tile}_same_bits"] = bool(torch.equal(y.view(torch.int32 if out_f32 else torch.int16),
                                                                y_ref.view(torch.int32 if out_f32 else torch.int16)))
            l.gsv_op_gemm_panel(C.byref(d), 1, 0, sp)
            code = int(l.gsv_debug_last_conv_route(1))
            row["auto_tile"] = f"{32 * (code >> 16 & 255)}x{32 * (code >> 24 & 255)}"
            best = min(row[f"tile{t}_us"] for t in (1, 2, 3))
            row["best_tflops"] = round(2 * M * K * N / best / 1e6, 1)
            print(json.dumps(row), flush=True)


def main():
    _lib.init(0)
    if "--panel" in sys.argv[1:]:
        return panel()
    shapes = [(934, 1024, 3072), (934, 1024, 1024), (934, 2048, 1024), (934, 1024, 2048), (5760, 512, 1536)]
    if len(sys.argv) > 1:
        shapes = [tuple(int(v) for v in a.split("x")) for a in sys.argv[1:]]
    for T, K, N in shapes:
        x = torch.randn(T, K, device="cuda", dtype=torch.float16)
        w = torch.randn(N, K, device="cuda", dtype=torch.float16) / K ** 0.5
        y = torch.zeros(T, N, device="cuda", dtype=torch.float16)
        d = _lib.ConvDesc(x.data_ptr(), w.data_ptr(), None, y.data_ptr(), None, T, T, K, N, 1, 1, 1, 0, 0, 0.0, 0, 1.0, 0, 0, 0, 0,
                          0, 0, 0, 0, 0, 0, 0, None)
        st = torch.cuda.current_stream()
        us = _time(lambda: _lib.lib().gsv_op_conv1d(C.byref(d), 1, C.c_void_p(st.cuda_stream)))
        print(json.dumps({"T": T, "K": K, "N": N, "us": round(us, 2), "tflops": round(2 * T * K * N / us / 1e6, 1),
                          "sk": "GSV_NO_GEMM_SK" not in os.environ}))


if __name__ == "__main__":
    main()
