"""GPU: gsv_op_token_logprob (csrc/t2s_sample.h token_logprob, one wave per row) against the fp64 mirror of _logprob_ref.py,
under the bar derived there from the arithmetic: 2**-23 * (32 + 2 |x_t - m| + |log S|).

Shapes: V = 1025 with Veff 1024 and 1025 (the 17th register of a lane holds one token) and V = 65 with Veff 64 (two registers).
Rows (B = 8): random at scale 3, all-equal logits (-log Veff), one logit at +80 among -80s, a row with -inf entries, a row whose
token sits 100 below the maximum, and copies of the first row at other positions (a row does not depend on its neighbours).
Tokens: 0, 63, 64, Veff - 1 and 1024 wherever the shape has them; a token in the masked EOS column gives -inf.
"""
import numpy as np
import pytest
import torch

from _logprob_ref import check_row, token_logprob_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 8
LOW = 7          # the token of row 4 that sits 100 below the row's maximum


def _rows(V, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, V, generator=g) * 3
    x[1] = 0.375
    x[2] = -80.0
    x[2, 11] = 80.0
    x[3, [2, 5, 62, V - 3]] = -float("inf")          # none of the tokens taken below
    x[4, LOW] = x[4].max() - 100.0
    x[5], x[7] = x[0], x[0]
    return x


def _op(x, V, Veff, tokens):
    from gsv import _lib
    _lib.init(0)
    xd = x.to(DEV).contiguous()
    td = torch.tensor(tokens, dtype=torch.int32, device=DEV)
    out = torch.full((B,), 123.0, dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().gsv_op_token_logprob(xd.data_ptr(), B, V, Veff, td.data_ptr(), out.data_ptr(), None),
               "gsv_op_token_logprob")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("V,Veff", [(1025, 1024), (1025, 1025), (65, 64)])
def test_op_matches_the_fp64_mirror(V, Veff):
    x = _rows(V, seed=V + Veff)
    xn = x.numpy()
    worst = 0.0
    for tok in sorted({0, 63, 64, Veff - 1, 1024} & set(range(V))):
        got = _op(x, V, Veff, [tok] * B)
        for b in range(B):
            worst = max(worst, check_row(got[b], xn[b], Veff, tok, f"V {V} Veff {Veff} row {b} token {tok}"))
        if tok >= Veff:                                     # the masked EOS column
            assert np.isneginf(got).all()
        else:
            assert np.isfinite(got).all()
        # the same row at positions 0, 5 and 7: equal bits
        assert got[0].tobytes() == got[5].tobytes() == got[7].tobytes()
    # per-row tokens: the argmax of every row, and row 4's token 100 below its maximum
    toks = [int(np.argmax(xn[b, :Veff])) for b in range(B)]
    toks[4] = LOW
    got = _op(x, V, Veff, toks)
    for b in range(B):
        worst = max(worst, check_row(got[b], xn[b], Veff, toks[b], f"V {V} Veff {Veff} row {b} token {toks[b]}"))
    assert abs(got[1] + np.log(Veff)) <= 2.0 ** -23 * (32 + np.log(Veff)), "all-equal logits: -log Veff"
    assert abs(got[2]) <= 2.0 ** -23 * 32, "one logit 160 above the rest holds all the mass"
    assert -101.0 - np.log(Veff) < got[4] < -100.0
    print(f"[token_logprob] V {V} Veff {Veff}: largest |error| / bar = {worst:.3f}")


def test_bad_arguments_are_refused():
    from gsv import _lib
    _lib.init(0)
    l = _lib.lib()
    x = torch.zeros(B, 65, device=DEV)
    t = torch.zeros(B, dtype=torch.int32, device=DEV)
    o = torch.zeros(B, device=DEV)
    assert l.gsv_op_token_logprob(x.data_ptr(), B, 65, 66, t.data_ptr(), o.data_ptr(), None) != 0
    assert l.gsv_op_token_logprob(x.data_ptr(), B, 4096, 64, t.data_ptr(), o.data_ptr(), None) != 0
    assert l.gsv_op_token_logprob(None, B, 65, 64, t.data_ptr(), o.data_ptr(), None) != 0
    assert l.gsv_op_token_logprob(x.data_ptr(), 0, 65, 64, t.data_ptr(), o.data_ptr(), None) != 0


def test_mirror_is_the_textbook_log_softmax():
    x = _rows(65, seed=1).double()
    ref = torch.log_softmax(x[0, :64], dim=-1)
    for tok in (0, 17, 63):
        assert abs(token_logprob_ref(x[0].numpy(), 64, tok)[0] - float(ref[tok])) < 1e-12
