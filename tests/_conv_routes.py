"""The conv / GEMM dispatch routes: a decoder for gsv_debug_last_conv_route and the table of cases that pins each route.

Every row names the kernel instantiation the DEFAULT dispatcher (no GSV_* environment switch) must pick for its shape and
says why.  tests/test_conv_routes_gpu.py runs each row against the fp64 mirror (tests/_convref.py); tests/test_conv_routes.py
checks on the CPU that the table reaches every instantiation in REACHABLE and nothing outside it.
"""
from __future__ import annotations

from dataclasses import dataclass, replace

FAMILY = {1: "gemm_sk", 2: "gemm_t64", 3: "conv_wide", 4: "gemm_lds", 5: "conv_lds", 6: "conv_narrow", 7: "conv_gemm", 8: "conv_pair"}
RES, ACCU, ALLW, WNT = 1, 2, 4, 8


def decode_route(code: int) -> str:
    """gsv_debug_last_conv_route's 64-bit record (byte fields, include/gsv.h) -> a readable instantiation name"""
    if code == 0:
        return "none"
    b = [(code >> (8 * i)) & 255 for i in range(8)]
    fam, dt, p, fl = b[0], ("f16" if b[1] == 1 else "f32"), b[2:7], b[7]
    r, a, al, nt = int(bool(fl & RES)), int(bool(fl & ACCU)), int(bool(fl & ALLW)), int(bool(fl & WNT))
    if fam == 1:
        return "gemm_sk_f16"
    if fam == 2:
        return f"gemm_t64_f16<WNT{nt},SLAB{16 * p[0]}>"
    if fam == 3:
        return f"conv_wide_f16<RES{r},ACC{a},W{p[0]}>"
    if fam == 4:
        return f"gemm_lds<{dt},RES{r},WNT{nt},W{p[0]},XCD{p[1]}>"
    if fam == 5:
        return f"conv_lds<{dt},TM{p[0]},TN{p[1]},WM{p[2]},WN{p[3]},CC{p[4]},ALLW{al},RES{r},ACC{a}>"
    if fam == 6:
        return f"conv_narrow_f16<CC{p[0]},TM{p[1]},TN{p[2]},WN{p[3]},RES{r},ACC{a}>"
    if fam == 7:
        return f"conv_gemm<{dt},TM{p[0]},TN{p[1]},WM{p[2]},WN{p[3]}>"
    if fam == 8:
        return f"conv_pair_f16<C{p[0]},TAPS{p[1]},ACC{a}>"
    return f"unknown({code:#x})"


def strip_xcd(route: str) -> str:
    """gemm_lds instantiation without the run-time xcd_order field"""
    return route.split(",XCD")[0] + ">" if route.startswith("gemm_lds<") else route


# ---- route names as the decoder prints them
def t64(wnt): return f"gemm_t64_f16<WNT{wnt},SLAB128>"
def wide(r, a): return f"conv_wide_f16<RES{r},ACC{a},W8>"
def glds(dt, r, nt, w, xcd): return f"gemm_lds<{dt},RES{r},WNT{nt},W{w},XCD{xcd}>"
def clds(dt, tm, tn, wm, wn, cc, allw, r, a): return f"conv_lds<{dt},TM{tm},TN{tn},WM{wm},WN{wn},CC{cc},ALLW{allw},RES{r},ACC{a}>"
def narrow(cc, tm, tn, wn, r, a): return f"conv_narrow_f16<CC{cc},TM{tm},TN{tn},WN{wn},RES{r},ACC{a}>"
def cg(dt, tm, tn, wm, wn): return f"conv_gemm<{dt},TM{tm},TN{tn},WM{wm},WN{wn}>"
def pair(c, taps, a): return f"conv_pair_f16<C{c},TAPS{taps},ACC{a}>"


SK = "gemm_sk_f16"
MODES = ((0, 0), (1, 0), (0, 1), (1, 1))     # (RES, ACCU)

# Every instantiation the default dispatcher can launch (gemm_lds without its run-time xcd_order), read from the launchers:
# gemm_sk.hip launch_gemm_sk, conv_wide.hip launch_conv_wide, gemm_lds.hip launch_gemm_lds, conv_narrow.hip launch_conv_narrow,
# conv_lds.hip launch_conv_lds, conv_gemm.hip launch_t, conv_pair.hip launch_pair_taps.  Not here, reached only through A/B
# switches (csrc/conv_launch.h ConvSwitches): gemm_t64 with
# SLAB 256 (GSV_T64_SLAB), conv_wide with 4 waves (GSV_WIDE_WAVES), the 4-wave fp16 conv_lds tiles (GSV_CONV_HALF_WAVES,
# GSV_CONV_TILE_WAVES); gemm_lds<f16,...,W4> IS default-reachable (grids of more than 256 tiles, Cin < 128).
REACHABLE = sorted(
    [SK, t64(0), t64(1)]
    + [wide(r, a) for r, a in MODES]
    + [strip_xcd(glds("f16", r, nt, w, 0)) for (r, nt) in ((0, 0), (1, 0), (0, 1)) for w in (4, 8)]
    + [strip_xcd(glds("f32", r, nt, 4, 0)) for (r, nt) in ((0, 0), (1, 0), (0, 1))]
    + [clds("f16", *g, cc, 0, r, a) for g in ((2, 1, 2, 4), (2, 2, 2, 4)) for cc in (128, 64) for r, a in MODES]
    + [clds("f32", *g, cc, 0, r, a) for g in ((2, 2, 2, 2), (2, 4, 2, 2)) for cc in (64, 32) for r, a in MODES]
    + [clds(dt, 2, 2, 1, 4, cc, 0, r, a) for dt in ("f16", "f32") for cc in (64, 32) for r, a in MODES]
    + [clds(dt, 1, 2, 1, 4, cc, 1, r, a) for dt in ("f16", "f32") for cc in (64, 32, 16) for r, a in MODES]
    + [narrow(cc, 1, 2, 4, r, a) for cc in (16, 32) for r, a in MODES] + [narrow(64, 2, 1, 8, r, a) for r, a in MODES]
    + [cg(dt, *g) for dt in ("f16", "f32") for g in ((1, 4, 1, 4), (1, 1, 2, 2), (2, 2, 1, 4), (2, 2, 2, 2))]
    + [pair(c, k, a) for c in (16, 32) for k in (3, 5, 7, 9, 11) for a in (0, 1)])

NONE, RELU, TANH, LRELU, SILU, GELU_TANH = 0, 1, 2, 3, 6, 8


@dataclass(frozen=True)
class Case:
    name: str
    route: str                 # expected decode_route() of the launch
    why: str                   # which dispatcher rule puts the shape there
    dtype: str = "f16"
    Cin: int = 64
    Cout: int = 64             # GEMM rows; with ups: ups * real output channels
    T: int = 300               # input rows; the output has T_out rows (= T at stride 1 with centred padding)
    taps: int = 3
    dil: int = 1
    stride: int = 1
    pad: int = -1              # -1: centred ((taps - 1) * |dil| // 2)
    pre: int = LRELU
    slope: float = 0.1
    post: int = NONE
    scale: float = 1.0
    res: bool = False
    acc: bool = False
    gate: bool = False
    out_f32: bool = False
    res_dtype: int = 0         # 0 follows out_f32, 1 fp32, 2 engine dtype
    y_col0: int = 0
    ldy: int = 0               # 0: y_col0 + real output channels
    Z: int = 1
    z_res: bool = False
    w_nt: bool = False
    ups: int = 0               # transposed conv: upsampling factor (dil = -1, pad = 0)
    ups_pad: int = 0


def _modes(base: Case, route_of, **kw):
    """the four RES / ACCU variants of one shape (accumulate with scale 1/3, the generator's MRF mean)"""
    out = []
    for r, a in MODES:
        out.append(replace(base, name=f"{base.name}_r{r}a{a}", route=route_of(r, a), res=bool(r), acc=bool(a),
                           scale=(1.0 / 3.0 if a else base.scale), **kw))
    return out


def _cases():
    C = Case
    L = []
    # ---------------- gemm_sk.hip: fp16 1 x 1, no pre-act / accumulate, Cin % 64 == 0 >= 256, Cout >= 64, T <= 2048, < 160 tiles
    L += [
        C("sk_res_gate_silu", SK, "Cin 320 is not a multiple of 512", Cin=320, Cout=200, T=77, taps=1, pre=NONE, post=SILU,
          res=True, gate=True),
        C("sk_cin576_odd_ldy", SK, "Cin 576 % 512 != 0; ldy 67 / y_col0 1: scalar row epilogue", Cin=576, Cout=64, T=65, taps=1,
          pre=NONE, res=True, y_col0=1, ldy=67),
        C("t64_gelu", t64(0), "Cin 512 % 512 == 0", Cin=512, Cout=96, T=100, taps=1, pre=NONE, post=GELU_TANH),
        C("t64_wnt_res_gate", t64(1), "w_nt selects the non-temporal weight loads", Cin=1024, Cout=128, T=63, taps=1, pre=NONE,
          res=True, gate=True, w_nt=True),
        C("t64_T2048", t64(0), "T_virt 2048 is the last skinny length", Cin=512, Cout=128, T=2048, taps=1, pre=NONE),
        C("glds_T2049", glds("f16", 0, 0, 8, 2), "T_virt 2049 > 2048 leaves gemm_sk; 17 tiles <= 256 -> 8 waves; T > 2 Cout",
          Cin=512, Cout=128, T=2049, taps=1, pre=NONE),
        C("sk_155_tiles", SK, "5 x 31 = 155 tiles < 160", Cin=256, Cout=3968, T=640, taps=1, pre=NONE),
        C("glds_160_tiles", glds("f16", 0, 0, 8, 1), "5 x 32 = 160 tiles leave gemm_sk; T <= 2 Cout -> XCD order 1",
          Cin=256, Cout=4096, T=640, taps=1, pre=NONE),
        C("t64_prefill_out32_res16", t64(0), "T2S prefill: fp32 output, fp16 residual", Cin=512, Cout=512, T=300, taps=1,
          pre=NONE, res=True, out_f32=True, res_dtype=2),
    ]
    # ---------------- gemm_lds.hip launch_gemm_lds: 1 x 1, T_virt >= 512, Cout >= 96, Cin >= BK
    L += [
        C("glds_prefill_out32_res16", glds("f16", 1, 0, 8, 2), "T2S prefill beyond 2048 tokens: fp32 out, fp16 residual",
          Cin=512, Cout=512, T=2100, taps=1, pre=NONE, res=True, out_f32=True, res_dtype=2),
        C("glds_wnt_w8", glds("f16", 0, 1, 8, 1), "pre-act leaves gemm_sk; 32 tiles; T 1024 == 2 Cout -> order 1", Cin=256,
          Cout=512, T=1024, taps=1, w_nt=True),
        C("glds_xcd2_cout511", glds("f16", 0, 0, 8, 2), "T 1024 > 2 x 511 -> XCD order 2; Cout tail 127", Cin=256, Cout=511,
          T=1024, taps=1),
        C("glds_xcd2_w3MB", glds("f16", 0, 0, 8, 2), "weights 256 x 6144 halfs = 3 MB (<= 3 MB) -> order 2", Cin=6144, Cout=256,
          T=600, taps=1),
        C("glds_xcd1_w3MB", glds("f16", 0, 0, 8, 1), "weights 256 x 6208 halfs > 3 MB -> order 1", Cin=6208, Cout=256, T=600,
          taps=1),
        C("glds_w4_cout96", glds("f16", 0, 0, 4, 2), "Cout 96 is the smallest GEMM tile user; Cin 64 < 128 -> 4 waves", Cin=64,
          Cout=96, T=600, taps=1, pre=NONE),
        C("clds_cout95", clds("f16", 2, 1, 2, 4, 64, 0, 0, 0), "Cout 95 < 96 -> conv_lds half tile (3 workgroups)", Cin=64,
          Cout=95, T=600, taps=1, pre=NONE),
        C("glds_w4_res", glds("f16", 1, 0, 4, 2), "Cin 112 < 128 -> 4 waves; residual", Cin=112, Cout=200, T=700, taps=1,
          pre=NONE, res=True),
        C("glds_w4_wnt", glds("f16", 0, 1, 4, 1), "Cin 64 -> 4 waves; w_nt; T 520 <= 2 x 384", Cin=64, Cout=384, T=520, taps=1,
          pre=NONE, w_nt=True),
        C("glds_256_tiles", glds("f16", 0, 0, 8, 2), "32 x 8 = 256 tiles -> still 8 waves", Cin=128, Cout=1024, T=4096, taps=1),
        C("glds_288_tiles", glds("f16", 0, 0, 4, 2), "32 x 9 = 288 tiles > 256 -> 4 waves", Cin=128, Cout=1025, T=4096, taps=1),
        C("glds_z2_zres", glds("f16", 1, 0, 8, 2), "Z = 2 with z_res (BWE): batched LDS GEMM with per-slice residual and bias",
          Cin=128, Cout=192, T=600, taps=1, pre=NONE, res=True, Z=2, z_res=True),
        C("cg_z2_res_no_zres", cg("f16", 1, 1, 2, 2), "Z = 2 with a residual but no z_res keeps the generic kernel; 20 tiles < 64",
          Cin=128, Cout=192, T=600, taps=1, pre=NONE, res=True, Z=2),
        C("glds_f32", glds("f32", 0, 0, 4, 2), "fp32 GEMM: always 4 waves", dtype="f32", Cin=96, Cout=160, T=600, taps=1, pre=NONE),
        C("glds_f32_res_gate", glds("f32", 1, 0, 4, 2), "fp32, residual + gate, T tail 1", dtype="f32", Cin=64, Cout=128, T=513,
          taps=1, pre=NONE, res=True, gate=True),
        C("glds_f32_wnt", glds("f32", 0, 1, 4, 1), "fp32, w_nt, T tail 127", dtype="f32", Cin=32, Cout=384, T=639, taps=1,
          pre=NONE, w_nt=True),
        C("clds_T511", clds("f16", 2, 1, 2, 4, 128, 0, 0, 0), "T_virt 511 < 512: not a GEMM tile shape", Cin=128, Cout=128,
          T=511, taps=1),
        C("glds_T512", glds("f16", 0, 0, 8, 2), "T_virt 512: GEMM tile", Cin=128, Cout=128, T=512, taps=1),
    ]
    # ---------------- conv_wide.hip: fp16, Cin = Cout = 128, T_virt >= 16384, span <= 50
    L += [
        C("wide_r0a0", wide(0, 0), "C 128, T 16384", Cin=128, Cout=128, T=16384, taps=3),
        C("wide_r1a0", wide(1, 0), "span 50 is the widest window; ragged last tile 255", Cin=128, Cout=128, T=16384 + 255, taps=11,
          dil=5, res=True),
        C("wide_r0a1", wide(0, 1), "accumulate, T tail 1", Cin=128, Cout=128, T=16385, taps=3, dil=3, acc=True, scale=1 / 3),
        C("wide_r1a1", wide(1, 1), "274 tiles > 256 workgroups: the persistent loop runs a second tile", Cin=128, Cout=128,
          T=70000, taps=2, dil=50, res=True, acc=True, scale=1 / 3),
        C("wide_T16383", clds("f16", 2, 1, 2, 4, 128, 0, 1, 0), "T 16383 < 16384 -> conv_lds half tile (64 workgroups)",
          Cin=128, Cout=128, T=16383, taps=3, res=True),
        C("span51", cg("f16", 2, 2, 2, 2), "span 51 > 50: neither wide nor LDS window; 128 tiles >= 64", Cin=128, Cout=128,
          T=16384, taps=2, dil=51, res=True),
    ]
    # ---------------- conv_lds_kernel, fp16: half tiles (Cout > 64, < 192 workgroups of 256 x 128)
    L += _modes(C("clds_half128", "", "Cout > 64, few workgroups, Cin >= 128; Cin 192 = 128 + 64 chunk tail", Cin=192, Cout=192,
                  T=333, taps=5, dil=2), lambda r, a: clds("f16", 2, 1, 2, 4, 128, 0, r, a))
    L += _modes(C("clds_half64", "", "64 <= Cin < 128; Cin 96 = 64 + 32 chunk tail; Cout 65 (tail 1)", Cin=96, Cout=65, T=257,
                  taps=7, dil=3), lambda r, a: clds("f16", 2, 1, 2, 4, 64, 0, r, a))
    L += [
        C("clds_T256", clds("f16", 2, 1, 2, 4, 64, 0, 1, 1), "T_virt 256 is the smallest LDS tile length", Cin=112, Cout=128,
          T=256, taps=3, res=True, acc=True, scale=0.5),
        C("cg_T255", cg("f16", 1, 1, 2, 2), "T_virt 255 < 256 -> generic; 2 tiles < 64", Cin=112, Cout=128, T=255, taps=3,
          res=True, acc=True, scale=0.5),
        C("clds_191_wgs", clds("f16", 2, 1, 2, 4, 128, 0, 0, 0), "15 x 12 = 180 workgroups < 192 -> half tile", Cin=128,
          Cout=1536, T=3840, taps=2),
    ]
    # full tiles (>= 192 workgroups)
    L += _modes(C("clds_full128", "", "16 x 12 = 192 workgroups", Cin=128, Cout=1536, T=4096, taps=2),
                lambda r, a: clds("f16", 2, 2, 2, 4, 128, 0, r, a))
    L += _modes(C("clds_full64", "", "192 workgroups, Cin 80 = 64 + 16 chunk tail, T tail 1", Cin=80, Cout=1536, T=3841 + 256,
                  taps=2), lambda r, a: clds("f16", 2, 2, 2, 4, 64, 0, r, a))
    # 64-channel tiles (32 < Cout <= 64)
    L += _modes(C("clds_c64_cc64", "", "Cout 33 > 32; Cin % 64 == 0", Cin=128, Cout=33, T=300, taps=5, dil=2),
                lambda r, a: clds("f16", 2, 2, 1, 4, 64, 0, r, a))
    L += _modes(C("clds_c64_cc32", "", "Cout 64; Cin 96 % 64 != 0 -> 32-channel chunks", Cin=96, Cout=64, T=511, taps=3),
                lambda r, a: clds("f16", 2, 2, 1, 4, 32, 0, r, a))
    L += [
        C("clds_c64_T16383", clds("f16", 2, 2, 1, 4, 64, 0, 0, 1), "T 16383 < 16384: not the persistent 64-channel kernel",
          Cin=64, Cout=48, T=16383, taps=3, acc=True, scale=1 / 3),
        C("cg_c48_cin48", cg("f16", 1, 1, 2, 2), "Cin 48 is neither a 64 nor a 32 multiple -> generic; 2 time tiles < 192",
          Cin=48, Cout=48, T=300, taps=3),
    ]
    # persistent 64-channel kernel
    L += _modes(C("narrow64", "", "Cin 64, Cout <= 64, T >= 16384; 547 tiles > 2 x 256 workgroups", Cin=64, Cout=64, T=140001,
                  taps=3), lambda r, a: narrow(64, 2, 1, 8, r, a))
    L += [C("narrow64_T16384", narrow(64, 2, 1, 8, 0, 0), "T 16384, Cout 48, span 50", Cin=64, Cout=48, T=16384, taps=11, dil=5)]
    # ALLW narrow tiles (Cout <= 32, all taps' weights in LDS)
    L += _modes(C("clds_allw64", "", "Cout 32; Cin % 64 == 0", Cin=128, Cout=32, T=1000, taps=5),
                lambda r, a: clds("f16", 1, 2, 1, 4, 64, 1, r, a))
    L += _modes(C("clds_allw32", "", "Cin 32, T 4095 < 4096: not persistent", Cin=32, Cout=20, T=4095, taps=11),
                lambda r, a: clds("f16", 1, 2, 1, 4, 32, 1, r, a))
    L += _modes(C("clds_allw16", "", "Cin 48 % 32 != 0", Cin=48, Cout=8, T=300, taps=3, dil=5),
                lambda r, a: clds("f16", 1, 2, 1, 4, 16, 1, r, a))
    L += [C("clds_allw16_cout1", clds("f16", 1, 2, 1, 4, 16, 1, 0, 0), "Cout 1, T 4095", Cin=16, Cout=1, T=4095, taps=3, dil=5)]
    # persistent 16 / 32-channel kernels
    L += _modes(C("narrow16", "", "Cin 16, T >= 4096; 782 tiles > 3 x 256 workgroups", Cin=16, Cout=16, T=200003, taps=11),
                lambda r, a: narrow(16, 1, 2, 4, r, a))
    L += _modes(C("narrow32", "", "Cin 32, T 4096, span 50", Cin=32, Cout=32, T=4096, taps=11, dil=5),
                lambda r, a: narrow(32, 1, 2, 4, r, a))
    L += [
        C("narrow16_conv_post", narrow(16, 1, 2, 4, 0, 0), "conv_post: Cout 1, fp32 output, tanh, lrelu 0.01", Cin=16, Cout=1,
          T=6000, taps=7, slope=0.01, post=TANH, out_f32=True),
        C("narrow32_odd_col", narrow(32, 1, 2, 4, 0, 0), "no epilogue operands: any slice; y_col0 3 -> scalar stores", Cin=32,
          Cout=13, T=4097, taps=3, y_col0=3, ldy=20),
    ]
    # ---------------- conv_lds_kernel, fp32 (64-wide chunks)
    L += _modes(C("f32_half64", "", "fp32 half tile, Cin 72 = 64 + 8", dtype="f32", Cin=72, Cout=130, T=300, taps=3),
                lambda r, a: clds("f32", 2, 2, 2, 2, 64, 0, r, a))
    L += _modes(C("f32_half32", "", "fp32 half tile, 32 <= Cin < 64", dtype="f32", Cin=40, Cout=96, T=383, taps=5),
                lambda r, a: clds("f32", 2, 2, 2, 2, 32, 0, r, a))
    L += _modes(C("f32_full64", "", "fp32 full tile, 192 workgroups", dtype="f32", Cin=64, Cout=1536, T=4096, taps=2),
                lambda r, a: clds("f32", 2, 4, 2, 2, 64, 0, r, a))
    L += _modes(C("f32_full32", "", "fp32 full tile, Cin 48", dtype="f32", Cin=48, Cout=1536, T=4096, taps=2),
                lambda r, a: clds("f32", 2, 4, 2, 2, 32, 0, r, a))
    L += _modes(C("f32_c64_cc64", "", "fp32 64-channel tile", dtype="f32", Cin=64, Cout=40, T=300, taps=3),
                lambda r, a: clds("f32", 2, 2, 1, 4, 64, 0, r, a))
    L += _modes(C("f32_c64_cc32", "", "fp32 64-channel tile, Cin 96", dtype="f32", Cin=96, Cout=64, T=257, taps=3),
                lambda r, a: clds("f32", 2, 2, 1, 4, 32, 0, r, a))
    L += _modes(C("f32_allw64", "", "fp32 ALLW, Cin 64, 3 taps fit", dtype="f32", Cin=64, Cout=32, T=700, taps=3),
                lambda r, a: clds("f32", 1, 2, 1, 4, 64, 1, r, a))
    L += _modes(C("f32_allw32", "", "fp32 ALLW, Cin 64 but 11 taps do not fit 64-wide chunks", dtype="f32", Cin=64, Cout=16,
                  T=300, taps=11, dil=5), lambda r, a: clds("f32", 1, 2, 1, 4, 32, 1, r, a))
    L += _modes(C("f32_allw16", "", "fp32 ALLW, Cin 16", dtype="f32", Cin=16, Cout=1, T=4096, taps=7),
                lambda r, a: clds("f32", 1, 2, 1, 4, 16, 1, r, a))
    # ---------------- conv_gemm.hip generic tilings
    for dt in ("f16", "f32"):
        L += [
            C(f"cg_{dt}_cout32", cg(dt, 1, 4, 1, 4), "Cout <= 32; stride 2 (LDS paths need stride 1)", dtype=dt, Cin=32, Cout=32,
              T=1001, taps=4, stride=2, pad=1),
            C(f"cg_{dt}_z191", cg(dt, 1, 1, 2, 2), "Cout 64, 1 x 191 tiles < 192", dtype=dt, Cin=32, Cout=64, T=256, taps=1,
              pre=NONE, Z=191),
            C(f"cg_{dt}_z192", cg(dt, 2, 2, 1, 4), "Cout 64, 1 x 192 tiles", dtype=dt, Cin=32, Cout=64, T=256, taps=1, pre=NONE,
              Z=192),
            C(f"cg_{dt}_63tiles", cg(dt, 1, 1, 2, 2), "stride 2, 63 tiles of 128 x 128 < 64", dtype=dt, Cin=32, Cout=128,
              T=2 * 8064, taps=4, stride=2, pad=1, res=True),
            C(f"cg_{dt}_64tiles", cg(dt, 2, 2, 2, 2), "stride 2, 64 tiles", dtype=dt, Cin=32, Cout=128, T=2 * 8192, taps=4,
              stride=2, pad=1, acc=True, scale=-1.0),
        ]
    L += [
        C("cg_f32_gate_res", cg("f32", 1, 1, 2, 2), "gate with taps > 1: only the generic kernel has it", dtype="f32", Cin=32,
          Cout=48, T=300, taps=3, res=True, gate=True),
        C("cg_f32_cout1_tanh", cg("f32", 1, 4, 1, 4), "Cout 1, fp32 tanh, T 255", dtype="f32", Cin=16, Cout=1, T=255, taps=7,
          post=TANH),
    ]
    # ---------------- transposed convs (polyphase scatter) and production slices
    L += [
        C("ups2_col2", clds("f16", 2, 2, 1, 4, 64, 0, 0, 0), "u 2, 64 virtual channels: 64-channel tile; y_col0 2 -> scalar",
          Cin=64, Cout=2 * 32, T=1000, taps=2, dil=-1, pad=0, ups=2, ups_pad=1, y_col0=2, ldy=40),
        C("ups8", clds("f16", 2, 1, 2, 4, 128, 0, 1, 0), "u 8, 512 virtual channels, residual rows scattered", Cin=128,
          Cout=8 * 64, T=300, taps=2, dil=-1, pad=0, ups=8, ups_pad=4, res=True),
        C("ups2_f32_generic", cg("f32", 1, 1, 2, 2), "T_virt 101 < 256 -> generic; y_col0 1", dtype="f32", Cin=32, Cout=2 * 32,
          T=100, taps=2, dil=-1, pad=0, ups=2, ups_pad=1, y_col0=1, ldy=35),
        C("clds_c64_odd_ldy_scale", clds("f16", 2, 2, 1, 4, 64, 0, 1, 1), "64-channel tile, y_col0 1 / ldy 70: scalar epilogue",
          Cin=64, Cout=64, T=400, taps=3, res=True, acc=True, scale=-0.5, y_col0=1, ldy=70),
        C("cg_f16_odd_ldy_scale", cg("f16", 1, 1, 2, 2), "generic kernel, y_col0 3 / ldy 135: scalar epilogue", Cin=32, Cout=128,
          T=2 * 1000, taps=4, stride=2, pad=1, res=True, scale=0.75, y_col0=3, ldy=135),
        C("flow_x1_minus_post", clds("f16", 2, 1, 2, 4, 128, 0, 0, 1), "the flow's x1 -= post(h): y_col0 96, scale -1, accumulate",
          Cin=192, Cout=96, T=300, taps=1, pre=NONE, scale=-1.0, acc=True, y_col0=96, ldy=192),
    ]
    return L


CASES = _cases()

# ---------------- conv_pair.hip: fused ResBlock pairs, every instantiation
PAIR_CASES = [(c, k, a, (196613 if (c, k, a) == (16, 3, 0) else 1000 + 37 * k + c), (1 if k >= 9 else 3 if k == 7 else 5))
              for c in (16, 32) for k in (3, 5, 7, 9, 11) for a in (0, 1)]    # (C, taps, accumulate, T, dil)
