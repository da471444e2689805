"""Shared by tests/test_gemm_panel.py (CPU) and tests/test_gemm_panel_gpu.py: the panel GEMM's tile family, its three epilogue
forms and the descriptor forms gsv_op_gemm_panel must refuse (include/gsv.h)."""
from __future__ import annotations

ACT_NONE, ACT_RELU, ACT_TANH, ACT_LRELU = 0, 1, 2, 3
GSV_F32, GSV_F16 = 0, 1
GSV_ERR_ARG = -1
ROUTE_GEMM_PANEL = 9

# forced `tile` -> (rows, output channels) of the tile (gemm_lds' summation)
TILES = {1: (192, 256), 2: (192, 192), 3: (96, 128)}
T64_TILE = 4                                          # the 96 x 128 tile with gemm_t64's two-accumulator summation (route p2 = 1)
# form -> (out_f32, residual, post_act): exactly what the prefill passes
FORMS = {"bias": (0, False, ACT_NONE), "bias_relu": (0, False, ACT_RELU), "bias_res_f32": (1, True, ACT_NONE)}


def desc_fields(form, M, K, N):
    """descriptor fields of an ELIGIBLE launch of `form` (pointers are filled in by the caller)"""
    out_f32, res, post = FORMS[form]
    return dict(T_in=M, T_out=M, Cin=K, Cout=N, taps=1, stride=1, dil=1, pad=0, pre_act=ACT_NONE, pre_slope=0.1, post_act=post,
                scale=1.0, accumulate=0, out_f32=out_f32, res_dtype=2 if res else 0)


# name -> (form the case starts from, descriptor overrides, dtype code, tile).  "x_off" / "w_off": bytes added to the pointer.
REFUSALS = {
    "fp32_engine": ("bias", {}, GSV_F32, 0),
    "gate": ("bias", {"gate": True}, GSV_F16, 0),
    "accumulate": ("bias", {"accumulate": 1}, GSV_F16, 0),
    "pre_activation": ("bias", {"pre_act": ACT_LRELU}, GSV_F16, 0),
    "batched_Z2": ("bias", {"Z": 2}, GSV_F16, 0),
    "misaligned_x": ("bias", {"x_off": 2}, GSV_F16, 0),
    "misaligned_w": ("bias", {"w_off": 8}, GSV_F16, 0),
    "misaligned_ldx": ("bias", {"ldx": 516}, GSV_F16, 0),
    "K_not_64": ("bias", {"Cin": 480}, GSV_F16, 0),
    "y_col0": ("bias", {"y_col0": 8, "ldy": 1024}, GSV_F16, 0),
    "taps3": ("bias", {"taps": 3, "pad": 1}, GSV_F16, 0),
    "tanh": ("bias", {"post_act": ACT_TANH}, GSV_F16, 0),
    "f32_out_without_residual": ("bias", {"out_f32": 1}, GSV_F16, 0),
    "residual_with_f16_out": ("bias_res_f32", {"out_f32": 0}, GSV_F16, 0),
    "f32_residual": ("bias_res_f32", {"res_dtype": 1}, GSV_F16, 0),
    "residual_relu": ("bias_res_f32", {"post_act": ACT_RELU}, GSV_F16, 0),
    "no_bias": ("bias", {"bias": None}, GSV_F16, 0),
    "unknown_tile": ("bias", {}, GSV_F16, 5),
    "negative_tile": ("bias", {}, GSV_F16, -1),
}


def refusal_desc(_lib, name, M, K, N, x, w, bias, y, res, gate):
    """(ConvDesc, dtype, tile) of refusal case `name`; x .. gate are device addresses (or any non-null numbers on the CPU)"""
    form, over, dtype, tile = REFUSALS[name]
    f = desc_fields(form, M, K, N)
    over = dict(over)
    x += over.pop("x_off", 0)
    w += over.pop("w_off", 0)
    g = gate if over.pop("gate", False) else None
    if "bias" in over:
        bias = over.pop("bias")
    f.update(over)
    d = _lib.ConvDesc(x=x, w=w, bias=bias, y=y, res=res if FORMS[form][1] else None, gate=g, **f)
    return d, dtype, tile
