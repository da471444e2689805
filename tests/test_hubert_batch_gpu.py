"""GPU: HubertModel.batch, many audios in one packed HuBERT pass, full-size synthetic weights (seed 0),
against the torch fp32 mirror tests/_hubert_ref.py (pinned to tests/golden/hubert_base.npz by tests/test_hubert_pack.py) and,
for the golden's own audio, against the golden.

Eight audios of 400, 719, 720, 20800, 41600, 8000, 48079 and 640 samples (sum T = 371), every audio compared on its own: a pooled
rms would hide an error confined to the one-frame audios.

Final features, per audio: relative rms <= 5e-3 and max-abs <= 3e-2, the bars test_hubert_matches_transformers_model holds the
per-audio engine to.

Stages.  With these weights the final features barely move from frame to frame (adjacent rows differ by 2.4 % of the rms), so
the final bars catch a wrong audio or key set but not a one-row slip at a segment edge.  The stages do: adjacent rows of "enc_in"
differ by at least 36 % of its rms, those of "pos" by at least 90 % of its own rms (0.076).  Both are pinned per audio (relative
rms of the difference) and per row (rms over the 768 channels of one row's difference, relative to the reference's rms over the
audio set).  The bars are twice the largest value the per-audio __call__(stages=...) -- the parent commit's arithmetic -- shows
against the mirror on the same eight audios:
  per-audio path, largest of 8 audios (MI355X): enc_in relative rms 1.304e-3, per-row 1.569e-3; pos relative rms 1.301e-3, per-row 1.672e-3
  bars:                                         enc_in 2.61e-3 and 3.14e-3; pos 2.61e-3 and 3.35e-3
  packed pass, largest of 8 audios (one pass, reversed order and three passes alike): enc_in 1.311e-3 and 1.608e-3; pos 1.304e-3
  and 1.674e-3; final features relative rms 1.37e-3 to 2.64e-3, max-abs 6.3e-3 to 8.7e-3 (per-audio path on the 8000-sample audio:
  1.51e-3, 6.0e-3; the packed pass on it: 1.48e-3, 7.8e-3)
A per-row bar of half the smallest adjacent-row distance (0.18 for enc_in, 0.45 for pos) or more would make the test blind; the
bars are 50 and 130 times below that."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import _hubert_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

FINAL_RMS, FINAL_ABS = 5e-3, 3e-2
# twice the per-audio path's largest figures (docstring): per-audio relative rms, per-row relative rms
STAGE_BARS = {"enc_in": (2.61e-3, 3.14e-3), "pos": (2.61e-3, 3.35e-3)}


@pytest.fixture(scope="module")
def model():
    from gsv import synthetic as S
    from gsv.feature_extractor.cnhubert import CNHubert
    return CNHubert(device=DEV, state_dict=S.make_hubert_state_dict(seed=0))


@pytest.fixture(scope="module")
def refs():
    """the mirror's outputs for the eight audios, computed once and left unchanged; the golden's audio carries the golden itself"""
    from gsv import synthetic as S
    sd = S.make_hubert_state_dict(seed=0)
    wavs = R.waveforms()
    out = [{k: v.numpy() for k, v in R.hubert(sd, w).items()} for w in wavs]
    out[R.GOLDEN_INDEX]["golden"] = load_golden("hubert_base")["last_hidden_state"].astype(np.float32)
    scale = {k: float(np.sqrt(np.mean(np.concatenate([o[k] for o in out]) ** 2))) for k in ("pos", "enc_in")}
    return wavs, out, scale


def _final(o, ref):
    d = o - ref
    return float(np.sqrt((d ** 2).mean() / (ref ** 2).mean())), float(np.abs(d).max())


def _stage(o, ref, scale):
    """(relative rms of the difference over the audio, largest per-row rms of the difference / the stage's rms)"""
    d = o - ref
    return float(np.sqrt((d ** 2).mean() / (ref ** 2).mean())), float(np.sqrt((d ** 2).mean(1)).max() / scale)


def _check(tag, outs, stages, refs, order=None):
    """prints every figure, then asserts the bars, audio by audio"""
    wavs, ref, scale = refs
    order = list(range(len(ref))) if order is None else order
    lens = [ref[i]["last_hidden_state"].shape[0] for i in order]
    assert [tuple(o.shape) for o in outs] == [(1, t, 768) for t in lens]
    assert all(o.dtype == torch.float16 and o.device.type == "cuda" for o in outs)
    rows, row0 = [], 0
    for i, t in zip(order, lens):
        rows.append((i, row0, t))
        row0 += t
    bad = []
    for (i, r0, t), o in zip(rows, outs):
        o = o[0].float().cpu().numpy()
        target = ref[i].get("golden", ref[i]["last_hidden_state"])
        rel, err = _final(o, target)
        line = f"[hubert batch] {tag} audio {i} (n = {R.LENGTHS[i]}, T = {t}): final rel rms {rel:.3e} max-abs {err:.3e}"
        if not (rel <= FINAL_RMS and err <= FINAL_ABS):
            bad.append(line)
        if stages is not None:
            for key in ("enc_in", "pos"):
                assert tuple(stages[key].shape) == (row0, 768) and stages[key].dtype == torch.float16
                a, b = _stage(stages[key][r0:r0 + t].float().cpu().numpy(), ref[i][key], scale[key])
                line += f"; {key} rel rms {a:.3e} per-row {b:.3e}"
                if not (a <= STAGE_BARS[key][0] and b <= STAGE_BARS[key][1]):
                    bad.append(f"{key} of audio {i}: {a:.3e} / {b:.3e}")
        print(line)
    assert not bad, bad


def test_per_audio_call_fills_stages(model, refs):
    """the per-audio path's own figures, the basis of STAGE_BARS: __call__(stages=...) on each audio against the mirror"""
    wavs, ref, scale = refs
    worst = {"enc_in": [0.0, 0.0], "pos": [0.0, 0.0]}
    for i, w in enumerate(wavs):
        st = {}
        out = model.model(w.unsqueeze(0).to(DEV), stages=st)["last_hidden_state"]
        assert sorted(st) == ["enc_in", "pos"]
        for key in ("enc_in", "pos"):
            assert tuple(st[key].shape) == (out.shape[1], 768) and st[key].dtype == torch.float16
            a, b = _stage(st[key].float().cpu().numpy(), ref[i][key], scale[key])
            worst[key] = [max(worst[key][0], a), max(worst[key][1], b)]
        rel, err = _final(out[0].float().cpu().numpy(), ref[i].get("golden", ref[i]["last_hidden_state"]))
        assert rel <= FINAL_RMS and err <= FINAL_ABS
    print(f"[hubert batch] per-audio __call__ vs mirror, largest over 8 audios: enc_in rel rms {worst['enc_in'][0]:.3e} per-row "
          f"{worst['enc_in'][1]:.3e}; pos rel rms {worst['pos'][0]:.3e} per-row {worst['pos'][1]:.3e}")
    for key in worst:
        assert worst[key][0] <= STAGE_BARS[key][0] / 2 and worst[key][1] <= STAGE_BARS[key][1] / 2, "the bars are twice what this path shows"
        assert STAGE_BARS[key][1] < (0.18 if key == "enc_in" else 0.45)


def test_batch_of_eight_audios(model, refs):
    """5a + 5b: one pass, every audio and both stages within the bars"""
    wavs, ref, _ = refs
    m = model.model
    before = m.passes
    stages = {}
    outs = model.batch(wavs, stages=stages)
    assert m.passes == before + 1 and m.last_pass_audios == 8 and sorted(stages) == ["enc_in", "pos"]
    assert sum(o.shape[1] for o in outs) == 371
    _check("one pass", outs, stages, refs)


def test_order_and_passes(model, refs):
    """5c: reversed input order, then three passes: the bars hold, outputs follow the inputs, passes rises by 1 and by 3"""
    wavs, ref, _ = refs
    m = model.model
    order = list(range(8))[::-1]
    before = m.passes
    stages = {}
    outs = m.batch([wavs[i].to(DEV) for i in order], stages=stages)           # device waveforms this time
    assert m.passes == before + 1
    _check("reversed", outs, stages, refs, order)
    stages = {}
    outs = m.batch(wavs, max_samples=50000, stages=stages)
    assert m.passes == before + 4
    _check("three passes", outs, stages, refs)


def test_single_audio_and_errors(model, refs):
    """5d"""
    wavs, ref, _ = refs
    m = model.model
    i = 5                                                                     # 8000 samples, T = 24
    w = wavs[i].unsqueeze(0)
    one = m.batch([w])
    assert len(one) == 1
    call = m(w.to(DEV))["last_hidden_state"]
    for tag, o in (("batch([w])", one[0]), ("model(w)", call)):
        rel, err = _final(o[0].float().cpu().numpy(), ref[i]["last_hidden_state"])
        print(f"[hubert batch] {tag}: final rel rms {rel:.3e} max-abs {err:.3e}")
        assert tuple(o.shape) == (1, 24, 768) and rel <= FINAL_RMS and err <= FINAL_ABS
    assert m.batch([]) == []
    before = m.passes
    from gsv import _lib
    _lib.lib().gsv_debug_last_conv_route(1)
    with pytest.raises(ValueError):
        m.batch([wavs[5], wavs[0][:399]])
    assert m.passes == before and _lib.lib().gsv_debug_last_conv_route(0) == 0      # refused before any launch
    a = m.batch(wavs[:4])
    b = m.batch(wavs[:4])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
