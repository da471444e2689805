"""GPU: per-row gates (ConvArgs::gate_rows / gate_ld, gsv_conv_desc.gate_rows) on every route the DiT's gated GEMMs can take --
gemm_sk, gemm_t64, gemm_lds (fp16 with 8 and with 4 waves, fp32) and the generic conv_gemm kernel -- with a DIFFERENT gate
vector per utterance, at row counts where an utterance boundary falls inside a tile (gate_rows = 934 or 40, tiles of 64 / 128
rows).  Each launch is held to an fp64 reference, gsv_debug_last_conv_route must name the family and carry flag 32 (GROWS),
and the reference with the lookup shifted by one row must miss the bar by far (the bar can see an index slip).

Bar, from the number formats: the products are exact in fp32 (fp16 operands) or rounded once (fp32), the K-term sum is kept in
fp32: worst case K * 2^-24 * sum |x w| <= K * 2^-24 * sqrt(K) with |x| <= 1, |w| <= 1 / sqrt(K), times the largest gate; plus
the bias / gate / residual roundings (a few 2^-24 |value|) and, for an fp16 output, 2^-11 |y| for the store."""
import ctypes as C

import pytest
import torch

from _conv_routes import decode_route
from gsv import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GROWS = 32

#        name            dtype  rows_per_gate  utterances  Cin   Cout  expected route (family, waves or None)
CASES = [("sk", "f16", 40, 3, 320, 128, (1, None)),                  # Cin % 512 != 0: the streaming split-K kernel
         ("t64_out", "f16", 934, 2, 1024, 1024, (2, None)),           # out-projection at 2 x 934 rows
         ("lds_w8_out", "f16", 934, 3, 1024, 1024, (4, 8)),           # 2802 rows > 2048, 22 x 8 = 176 tiles <= 256: 8 waves
         ("lds_w8_ff2", "f16", 934, 3, 2048, 1024, (4, 8)),           # FF2 (K = 2048) on the same route
         ("lds_w4_out", "f16", 934, 5, 1024, 1024, (4, 4)),           # 4670 rows, 37 x 8 = 296 tiles > 256: 4 waves
         ("lds_f32", "f32", 40, 13, 128, 128, (4, 4)),                # fp32 from 512 rows (13 x 40 = 520), Cout >= 96
         ("lds_f32_ff2", "f32", 40, 13, 256, 128, (4, 4)),
         ("generic_f32", "f32", 40, 3, 128, 128, (7, None)),          # below 512 rows: the generic kernel
         ("generic_f16", "f16", 40, 5, 128, 128, (7, None))]          # fp16, Cin < 256: neither gemm_sk nor (200 rows) gemm_lds


def _launch(dtype, x, w, bias, gate, res, y, rows, Cin, Cout, gate_rows, gate_ld):
    from gsv import _lib
    d = _lib.ConvDesc()
    d.x, d.w, d.bias, d.y, d.res, d.gate = x.data_ptr(), w.data_ptr(), bias.data_ptr(), y.data_ptr(), res.data_ptr(), gate.data_ptr()
    d.T_in = d.T_out = rows
    d.Cin, d.Cout, d.taps, d.stride, d.dil, d.pad = Cin, Cout, 1, 1, 1, 0
    d.scale, d.Z = 1.0, 1
    d.res_dtype = 2
    d.gate_rows, d.gate_ld = gate_rows, gate_ld
    lib = _lib.lib()
    lib.gsv_debug_last_conv_route(1)
    rc = lib.gsv_op_conv1d(C.byref(d), _lib.GSV_F16 if dtype == "f16" else _lib.GSV_F32, None)
    torch.cuda.synchronize()
    return rc, int(lib.gsv_debug_last_conv_route(1))


def dispatch_route(dtype, rows, Cin, Cout, gate_rows):
    """the route record (byte fields) of a gated GEMM with a residual and per-row gates at this shape, on zero data: the
    dispatcher's choice is a function of the descriptor alone"""
    from gsv import _lib
    _lib.init(0)
    td = torch.float16 if dtype == "f16" else torch.float32
    with torch.cuda.device(DEV):
        x, w = torch.zeros(rows, Cin, dtype=td, device=DEV), torch.zeros(Cout, Cin, dtype=td, device=DEV)
        b, g = torch.zeros(Cout, device=DEV), torch.ones((rows + gate_rows - 1) // gate_rows, Cout, device=DEV)
        r, y = torch.zeros(rows, Cout, dtype=td, device=DEV), torch.zeros(rows, Cout, dtype=td, device=DEV)
        rc, route = _launch(dtype, x, w, b, g, r, y, rows, Cin, Cout, gate_rows, Cout)
    assert rc == 0
    return [(route >> (8 * i)) & 255 for i in range(8)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_per_row_gates_on_every_route(case):
    name, dtype, gr, B, Cin, Cout, (family, waves) = case
    from gsv import _lib
    _lib.init(0)
    td = torch.float16 if dtype == "f16" else torch.float32
    R, ld = B * gr, Cout + 8                                      # gate_ld > Cout: a stride mistake shows
    x = S.hash_symmetric(f"gr_x_{name}", (R, Cin), 1.0, 1).to(td)
    w = (S.hash_symmetric(f"gr_w_{name}", (Cout, Cin), 1.0, 2) / Cin ** 0.5).to(td)
    bias = S.hash_symmetric(f"gr_b_{name}", (Cout,), 0.5, 3)
    res = S.hash_symmetric(f"gr_r_{name}", (R, Cout), 1.0, 4).to(td)
    # utterance b's gates lie in +-[2 b + 1, 2 b + 2): neighbours differ by at least 1 in every channel
    gate = torch.zeros(B, ld)
    for b in range(B):
        g = S.hash_symmetric(f"gr_g_{name}", (Cout,), 1.0, 10 + b)
        gate[b, :Cout] = torch.sign(g + 1e-3) * (2 * b + 1 + g.abs())
    gate[:, Cout:] = float("nan")                                 # the padding is never read
    with torch.cuda.device(DEV):
        guard = 4096
        y = torch.full((R * Cout + guard,), float("nan"), dtype=td, device=DEV)
        dev = [t.to(DEV).contiguous() for t in (x, w, bias, gate, res)]
        rc, route = _launch(dtype, dev[0], dev[1], dev[2], dev[3], dev[4], y, R, Cin, Cout, gr, ld)
    assert rc == 0
    b8 = [(route >> (8 * i)) & 255 for i in range(8)]
    print(f"{name}: route {decode_route(route)} flags {b8[7]:#x}")
    assert b8[0] == family and (b8[7] & GROWS), f"expected family {family} with the GROWS flag, got {decode_route(route)} flags {b8[7]:#x}"
    assert waves is None or b8[2] == waves, f"expected {waves} waves, got {b8[2]}"
    assert torch.isnan(y[R * Cout:].float()).all(), "the sentinels behind y"
    out = y[:R * Cout].view(R, Cout).double().cpu()
    acc = x.double() @ w.double().t() + bias.double()
    rows = torch.arange(R)

    def ref(shift):
        g = gate[((rows + shift).clamp(max=R - 1) // gr)][:, :Cout].double()
        return acc * g + res.double()
    want = ref(0)
    gmax = float(gate[:, :Cout].abs().max())
    bar = Cin ** 1.5 * 2.0 ** -24 * gmax + 8 * 2.0 ** -24 * (want.abs() + gmax) + (2.0 ** -11 * want.abs() if dtype == "f16" else 0.0)
    err = (out - want).abs()
    print(f"{name}: R {R}, max error {float(err.max()):.3e}, bar at that element {float(bar.flatten()[err.argmax()]):.3e}")
    assert torch.isfinite(out).all() and bool((err <= bar).all())
    # the bar sees a lookup that is one row off: only the B - 1 boundary rows differ, and they miss it by far
    slip = (ref(1) - want).abs()
    assert float((slip / bar).max()) > 20, "the case cannot see an index slip"
    # and per utterance block the gates really differ
    assert all(float((gate[b, :Cout] - gate[b + 1, :Cout]).abs().min()) >= 1.0 for b in range(B - 1))


def test_per_row_gates_are_refused_where_they_cannot_be_honoured():
    """gate_ld < Cout and a negative gate_rows are errors before anything is launched"""
    from gsv import _lib
    _lib.init(0)
    with torch.cuda.device(DEV):
        R, Cin, Cout = 80, 128, 128
        x = torch.zeros(R, Cin, device=DEV)
        w = torch.zeros(Cout, Cin, device=DEV)
        b = torch.zeros(Cout, device=DEV)
        g = torch.ones(2, Cout, device=DEV)
        r = torch.zeros(R, Cout, device=DEV)
        y = torch.full((R * Cout,), float("nan"), device=DEV)
        assert _launch("f32", x, w, b, g, r, y, R, Cin, Cout, 40, Cout - 4)[0] != 0
        assert _launch("f32", x, w, b, g, r, y, R, Cin, Cout, -1, Cout)[0] != 0
        assert torch.isnan(y).all()
        assert _launch("f32", x, w, b, g, r, y, R, Cin, Cout, 40, Cout)[0] == 0
        assert torch.isfinite(y).all()
