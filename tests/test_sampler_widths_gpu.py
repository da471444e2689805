"""GPU: every instantiation of the sampler (csrc/t2s.hip with_npl: 2, 17 or 32 values per lane for V <= 128, <= 1088, <= 2048)
at its boundaries, with Veff == V (every step after the EOS horizon) as well as Veff == V - 1.

gsv_op_sample_rows with injected noise against the oracle, row by row and integer-exact: the comparison, the nine settings
and the input recipe (ties, -inf, both zeros; tie-free and twice as wide for the top-p rows) of
test_row_sampling_gpu.test_sampler_rows_match_the_oracle_row_by_row, over 18 rows.  Rows 0 .. 8 are the recipe as it is; rows
9 .. 17 repeat the settings with plants:

* the maximum at token Veff - 1, the last token of the last used register, in the greedy row and the unfiltered row;
* in the top-k 2 row (no penalty) the k-th value tied between token 10 and the last token of the widest register the shape
  reaches (v >= 64 (NPL - 1) where Veff goes that far), the noise of that token the smallest of its row, so it is drawn if and
  only if the tie kept it; the top-k 5 row the same with five values.

The seeds of the inputs are chosen on the CPU so that the top-p guard (cumulative mass 1e-4 away from top_p) holds.

gsv_op_token_logprob at (2048, 2047) and (128, 128) against tests/_logprob_ref.py under its bar.  The bar's derivation counts 17
sequential additions per lane; with 32 the sum's error grows from 16 to 23.8 eps (38 additions at eps / 2, log(2048) / 2, expf),
still inside the 32 eps the bar allows before its |x_t - m| and |log S| terms.
"""
import numpy as np
import pytest
import torch

from _logprob_ref import check_row
from test_row_sampling_gpu import MARGIN, NINE, _oracle_row, _sampler_inputs, _top_p_margin
from test_token_logprob_op_gpu import B as LP_B, LOW, _op as _logprob_op, _rows as _logprob_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, PREV_LEN = 18, 24
SHAPES = [(64, 64), (65, 65), (128, 127), (128, 128), (129, 128), (1088, 1087), (1088, 1088), (1089, 1088), (1089, 1089),
          (2048, 2047), (2048, 2048)]
# input seed per shape, the first of 0, 1, 2, ... at which every top-p row keeps its margin (searched on the CPU)
SEED = {(64, 64): 0, (65, 65): 0, (128, 127): 0, (128, 128): 0, (129, 128): 0, (1088, 1087): 0, (1088, 1088): 0,
        (1089, 1088): 0, (1089, 1089): 0, (2048, 2047): 1, (2048, 2048): 1}
GREEDY, TOPK5, UNFILTERED, TOPK2 = 9 + 0, 9 + 1, 9 + 4, 9 + 8       # planted rows, by their setting in NINE


def npl(V):
    return 2 if V <= 128 else 17 if V <= 1088 else 32


def _inputs(V, Veff, seed):
    """the recipe's inputs with the plants; returns (logits, prev, noise, expected) with expected[row] = the token the row must
    draw, or its argmax for the unfiltered row"""
    logits, prev, noise = _sampler_inputs(V, B, PREV_LEN, seed)
    assert int(prev.max()) < Veff
    last = Veff - 1
    top = float(logits[torch.isfinite(logits)].max())
    logits[GREEDY, last] = top + 10.0                    # the maximum even after a penalty of 1.35
    # the unfiltered row: the maximum by 0.5 only, so that the draw stays open; the token is kept out of the row's history
    prev[UNFILTERED][prev[UNFILTERED] == last] = 0
    logits[UNFILTERED, last] = float(logits[UNFILTERED][torch.isfinite(logits[UNFILTERED])].max()) + 0.5
    assert NINE[TOPK2 % 9] == (2, 1.0, 1.0, 1.0) and NINE[TOPK5 % 9][0] == 5
    logits[TOPK2, 20], logits[TOPK2, 10], logits[TOPK2, last] = top + 2.0, top + 1.0, top + 1.0
    # five values: four above, the fifth tied between token 10 and the last token; none of them in the row's history
    prev[TOPK5] = 3
    logits[TOPK5, 20:24] = top + 2.0
    logits[TOPK5, 10], logits[TOPK5, last] = top + 1.0, top + 1.0
    for b in (TOPK2, TOPK5):
        noise[b, last] = 1e-6                            # p / q of the tied last token beats every other kept token
    return logits, prev, noise, {GREEDY: last, UNFILTERED: last, TOPK2: last, TOPK5: last}


def guard_ok(V, Veff, seed):
    """host: every top-p row of the shape's inputs keeps its margin"""
    logits, prev, _, _ = _inputs(V, Veff, seed)
    return all(_top_p_margin(logits[b, :Veff], prev[b], NINE[b % 9][3], NINE[b % 9][1]) >= MARGIN
               for b in range(B) if NINE[b % 9][1] < 1.0)


@pytest.mark.parametrize("V,Veff", SHAPES)
def test_sampler_rows_match_the_oracle_at_every_width(V, Veff):
    from gsv import _lib
    _lib.init(0)
    logits, prev, noise, expected = _inputs(V, Veff, SEED[(V, Veff)])
    settings = [NINE[b % 9] for b in range(B)]
    for b, (k, p, t, rp) in enumerate(settings):
        if p < 1.0:
            m = _top_p_margin(logits[b, :Veff], prev[b], rp, p)
            assert m >= MARGIN, f"bad input: row {b} (top_p {p}) has cumulative mass within {m:.2e} of top_p; pick another seed"
    ref = [_oracle_row(logits[b, :Veff], prev[b], noise[b], settings[b]) for b in range(B)]
    # the plants took: the oracle itself draws the last token there (the unfiltered row: its argmax)
    for b, tok in expected.items():
        assert ref[b][1 if b == UNFILTERED else 0] == tok, f"plant of row {b} did not take: oracle {ref[b]}"
    # the planted last token sits in the instance's last register, except where Veff ends before it: these four shapes
    assert Veff - 1 >= 64 * (npl(V) - 1) or (V, Veff) in ((64, 64), (129, 128), (1089, 1088), (1089, 1089))
    rows = (_lib.RowSampling * B)(*[_lib.RowSampling(*s) for s in settings])
    lg_d, pv_d, nz_d = logits.to(DEV).contiguous(), prev.to(DEV, torch.int32).contiguous(), noise.to(DEV).contiguous()
    out_s = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    out_a = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().gsv_op_sample_rows(lg_d.data_ptr(), B, V, Veff, pv_d.data_ptr(), PREV_LEN, rows, 0, nz_d.data_ptr(),
                                             0, out_s.data_ptr(), out_a.data_ptr(), None), "gsv_op_sample_rows")
    torch.cuda.synchronize()
    got = list(zip(out_s.cpu().tolist(), out_a.cpu().tolist()))
    for b in range(B):
        assert got[b] == ref[b], f"V {V} Veff {Veff} row {b} with {settings[b]}: (sample, argmax) {got[b]}, oracle {ref[b]}"


@pytest.mark.parametrize("V,Veff", [(2048, 2047), (128, 128)])
def test_token_logprob_at_the_widest_and_the_full_instance(V, Veff):
    x = _logprob_rows(V, seed=V + Veff)
    xn = x.numpy()
    worst = 0.0
    for tok in sorted({0, 63, 64, 127, 1984, Veff - 1, V - 1} & set(range(V))):
        got = _logprob_op(x, V, Veff, [tok] * LP_B)
        for b in range(LP_B):
            worst = max(worst, check_row(got[b], xn[b], Veff, tok, f"V {V} Veff {Veff} row {b} token {tok}"))
        assert np.isneginf(got).all() if tok >= Veff else np.isfinite(got).all()
        assert got[0].tobytes() == got[5].tobytes() == got[7].tobytes()
    toks = [int(np.argmax(xn[b, :Veff])) for b in range(LP_B)]
    toks[4] = LOW
    got = _logprob_op(x, V, Veff, toks)
    for b in range(LP_B):
        worst = max(worst, check_row(got[b], xn[b], Veff, toks[b], f"V {V} Veff {Veff} row {b} token {toks[b]}"))
    assert abs(got[1] + np.log(Veff)) <= 2.0 ** -23 * (32 + np.log(Veff)), "all-equal logits: -log Veff"
    print(f"[token_logprob] V {V} Veff {Veff}: largest |error| / bar = {worst:.3f}")
