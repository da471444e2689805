"""CPU: the layout of the packed HuBERT pass (HubertModel.pack_plan / pack_passes) and the torch mirror
the GPU tests compare against (tests/_hubert_ref.py)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import _hubert_ref as R


@pytest.fixture(scope="module")
def sd():
    from gsv import synthetic as S
    return S.make_hubert_state_dict(seed=0)


def test_mirror_matches_golden(sd):
    """the fp32 mirror against transformers.HubertModel's stored output on make_waveform(20800, 7).  The golden is stored as fp16:
    its own rounding is half an ulp at 2.68 = 9.8e-4 max-abs, 2.1e-4 relative rms (measured with a scratch mirror); bars 1.5e-3
    and 5e-4.  Measured here: max-abs 9.8e-4, relative rms 2.1e-4."""
    from gsv import synthetic as S
    ref = load_golden("hubert_base")["last_hidden_state"].astype(np.float32)
    out = R.hubert(sd, S.make_waveform(20800, 7))
    o = out["last_hidden_state"].numpy()
    assert o.shape == ref.shape == (64, 768) and out["pos"].shape == out["enc_in"].shape == (64, 768)
    err = np.abs(o - ref).max()
    rel = np.sqrt(((o - ref) ** 2).mean() / (ref ** 2).mean())
    print(f"[hubert mirror] vs golden: max-abs {err:.3e}, relative rms {rel:.3e}")
    assert err <= 1.5e-3 and rel <= 5e-4


def test_pack_plan_against_torch(sd):
    """the packed stream through the mirror's conv stack, GroupNorm per plan segment, against each audio's own stack in fp64:
    rows [k_s, k_s + T_s) agree to 1e-10; the row counts and the two gather index arrays are what the layout says"""
    from gsv.feature_extractor.cnhubert import HubertModel
    wavs = R.waveforms()
    plan = HubertModel.pack_plan(R.LENGTHS)
    assert plan["T"] == [(n - 400) // 320 + 1 for n in R.LENGTHS]
    assert plan["T0"] == [(n - 10) // 5 + 1 for n in R.LENGTHS]
    slots = [(n + 319) // 320 * 320 for n in R.LENGTHS]
    assert plan["samples"] == sum(slots) and plan["rows"] == sum(slots) // 320 - 1
    assert plan["slot_off"] == [sum(slots[:i]) for i in range(len(slots))]
    stream = torch.zeros(plan["samples"], dtype=torch.float64)
    for w, off in zip(wavs, plan["slot_off"]):
        stream[off:off + w.numel()] = w.double()
    packed = R.conv_stack(sd, stream, torch.float64, gn_segments=list(zip(plan["cn_start"], plan["cn_len"])))
    assert packed.shape[0] == plan["rows"]
    worst = 0.0
    for w, k, t in zip(wavs, plan["k"], plan["T"]):
        own = R.conv_stack(sd, w, torch.float64)
        assert own.shape[0] == t
        worst = max(worst, (packed[k:k + t] - own).abs().max().item())
    print(f"[hubert pack] packed conv stack vs per audio, fp64: max-abs {worst:.2e}")
    assert worst <= 1e-10
    # the padded layout: the audios' packed rows in order, exactly 64 entries of -1 between two audios and none at the ends
    gp, gd = plan["gather_pad"].tolist(), plan["gather_dense"].tolist()
    want = []
    for s, (k, t) in enumerate(zip(plan["k"], plan["T"])):
        want += ([-1] * 64 if s else []) + list(range(k, k + t))
    assert gp == want and gp[0] >= 0 and gp[-1] >= 0 and len(gp) == sum(plan["T"]) + 64 * (len(R.LENGTHS) - 1)
    # the dense layout: exactly the rows of the padded layout that belong to an audio, in order
    assert gd == [i for i, r in enumerate(gp) if r >= 0]
    assert [gp[i] for i in gd] == [r for k, t in zip(plan["k"], plan["T"]) for r in range(k, k + t)]
    assert plan["row0"] == [sum(plan["T"][:i]) for i in range(len(R.LENGTHS))]
    assert plan["gather_pad"].dtype == plan["gather_dense"].dtype == torch.int32
    # the rest of the layout in torch, fp64: projection on all packed rows, the audios 64 zero rows apart through ONE positional
    # conv, LayerNorm, dense gather -- against each audio's own positional conv and LayerNorm
    proj = R.feature_projection(sd, packed, torch.float64)
    padded = torch.zeros(len(gp), proj.shape[1], dtype=torch.float64)
    keep = plan["gather_pad"] >= 0
    padded[keep] = proj[plan["gather_pad"][keep].long()]
    pos, enc_in = (t[plan["gather_dense"].long()] for t in R.positional(sd, padded, torch.float64))
    worst = 0.0
    for w, r0, t in zip(wavs, plan["row0"], plan["T"]):
        own_pos, own_in = R.positional(sd, R.feature_projection(sd, R.conv_stack(sd, w, torch.float64), torch.float64), torch.float64)
        worst = max(worst, (pos[r0:r0 + t] - own_pos).abs().max().item(), (enc_in[r0:r0 + t] - own_in).abs().max().item())
    print(f"[hubert pack] packed positional conv + LayerNorm vs per audio, fp64: max-abs {worst:.2e}")
    assert worst <= 1e-10


def test_pack_plan_errors_and_passes():
    from gsv.feature_extractor.cnhubert import HubertModel as H
    with pytest.raises(ValueError):
        H.pack_plan([399])
    with pytest.raises(ValueError):
        H.pack_passes([8000, 399], 2 ** 21)
    assert H.pack_passes([], 2 ** 21) == []
    # input order, never split, at most max_samples slot samples
    assert H.pack_passes(R.LENGTHS, 50000) == [[0, 1, 2, 3], [4, 5], [6, 7]]
    assert H.pack_passes(R.LENGTHS) == [list(range(8))]
    # an audio longer than max_samples gets a pass of its own as long as it fits the bound of one pass
    assert H.pack_passes([8000, 100000, 8000], 16000) == [[0], [1], [2]]
    big = H.PASS_LIMIT - 320
    assert H.pack_passes([8000, big, 8000], 2 ** 21) == [[0], [1], [2]]
    plan = H.pack_plan([big])
    assert plan["samples"] == big and plan["rows0"] * 512 < 2 ** 31 and plan["T"] == [(big - 400) // 320 + 1]
    with pytest.raises(ValueError):
        H.pack_passes([8000, H.PASS_LIMIT], 2 ** 21)
    with pytest.raises(ValueError):
        H.pack_plan([H.PASS_LIMIT])
    with pytest.raises(ValueError):
        H.pack_plan([big, 8000])
    # at most MAX_AUDIOS audios per pass
    assert [len(g) for g in H.pack_passes([400] * (H.MAX_AUDIOS + 1), H.PASS_LIMIT - 1)] == [H.MAX_AUDIOS, 1]
