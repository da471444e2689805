"""CPU: the AP-BWE super-sampling front door (gsv/tools/audio_sr.py) -- checkpoint / config.json loading, the missing
checkpoint error, the synthetic state dict against the reference's APNet_BWE_Model schema recorded in the fixtures, the
resampler restatement, and the new library exports.  No GPU compute is called here."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from gsv import synthetic as S


@pytest.mark.parametrize("fixture,config", [("bwe_small", S.small_bwe_config()), ("bwe_full", S.BWE_24K_48K_CONFIG)])
def test_state_dict_schema_matches_reference_model(fixture, config):
    g = load_golden(fixture)
    assert json.loads(str(g["config"])) == config
    ref = json.loads(str(g["sd_schema"]))
    sd = S.make_bwe_state_dict(config, int(g["seed"]))
    assert sorted(sd) == sorted(ref)
    for k, v in sd.items():
        assert list(v.shape) == ref[k], k
    L = config["ConvNeXt_layers"]
    gam = torch.stack([sd[f"convnext_mag.{i}.gamma"] for i in range(L)])
    assert abs(gam.mean().item() - 1.0 / L) < 0.05 / L                 # layer_scale_init_value = 1 / L (model.py:82)


def test_state_dict_is_deterministic():
    a, b = S.make_bwe_state_dict(S.small_bwe_config(), 0), S.make_bwe_state_dict(S.small_bwe_config(), 0)
    assert all(torch.equal(a[k], b[k]) for k in a)
    c = S.make_bwe_state_dict(S.small_bwe_config(), 1)
    assert not torch.equal(a["conv_pre_mag.weight"], c["conv_pre_mag.weight"])


def test_missing_checkpoint_names_the_path(tmp_path):
    from gsv.tools.audio_sr import AP_BWE
    path = str(tmp_path / "nowhere" / "g_24kto48k.zip")
    with pytest.raises(FileNotFoundError, match="nowhere/g_24kto48k.zip"):
        AP_BWE("cuda:0", checkpoint_file=path)


def test_checkpoint_and_config_json_are_read(tmp_path, monkeypatch):
    """a torch.save({"generator": sd}) file with config.json beside it: the config reaches the engine, the state dict loads
    with weights_only=True, and a CPU device is refused (there is no CPU path)"""
    from gsv.tools import audio_sr
    cfg = S.small_bwe_config()
    sd = S.make_bwe_state_dict(cfg, 0)
    torch.save({"generator": sd}, tmp_path / "g.pt")
    (tmp_path / "config.json").write_text(json.dumps(cfg))
    seen = {}

    def fake_to(self, device=None, dtype=None):
        seen["device"], seen["dtype"] = device, self.dtype
        return self

    monkeypatch.setattr(audio_sr.AP_BWE, "to", fake_to)
    m = audio_sr.AP_BWE("cuda:0", checkpoint_file=str(tmp_path / "g.pt"))
    assert m.config == cfg and seen == {"device": "cuda:0", "dtype": torch.float32}
    assert sorted(m._sd) == sorted(sd) and all(torch.equal(m._sd[k], sd[k]) for k in sd)
    class Attr(dict):
        __getattr__ = dict.__getitem__
    m2 = audio_sr.AP_BWE("cuda:0", Attr, state={"generator": sd}, config=cfg, dtype=torch.float16)
    assert m2.h.n_fft == cfg["n_fft"] and m2.dtype == torch.float16
    assert m.out_len(2400, 24000) == 4800 and m.out_len(3200, 32000) == 4800 and m.out_len(2001, 24000) == 4000
    with pytest.raises(ValueError):
        m.out_len(64, 24000)                 # 128 samples at 48 kHz: not more than the reflect padding of n_fft / 2
    monkeypatch.undo()
    with pytest.raises(RuntimeError):
        audio_sr.AP_BWE("cpu", state={"generator": sd}, config=cfg)


def test_resample_restatement_matches_fixture_and_is_band_limited():
    from gsv.tools.audio_sr import resample
    g = load_golden("bwe_small")
    y = resample(S.make_bwe_input("bwe_in_small", 2400, gap=(900, 1620)), 24000, 48000)
    assert y.shape == (1, 4800)
    np.testing.assert_array_equal(y[0].numpy(), g["resampled"])
    # a 1 kHz tone stays a 1 kHz tone of the same amplitude (away from the edges)
    t = torch.arange(3200, dtype=torch.float64) / 32000
    z = resample(torch.sin(2 * np.pi * 1000 * t).float().view(1, -1), 32000, 48000)[0]
    ref = torch.sin(2 * np.pi * 1000 * torch.arange(4800, dtype=torch.float64) / 48000).float()
    assert z.shape[0] == 4800 and (z - ref)[200:-200].abs().max() < 2e-2


def test_inverse_dft_basis_inverts_the_forward_basis():
    """windowed irfft basis: irfft(rfft(x w) ) w sums back to x w^2; DC / Nyquist imaginary columns are zero"""
    from gsv.module.mel_processing import _dft_basis
    n_fft, win = 64, 32
    fw = _dft_basis(n_fft, win, "cpu").double()
    iv = _dft_basis(n_fft, win, "cpu", inverse=True).double()
    bins = n_fft // 2 + 1
    assert iv.shape == (n_fft, 2 * bins) and iv[:, bins].abs().max() == 0 and iv[:, 2 * bins - 1].abs().max() == 0
    x = torch.randn(n_fft, dtype=torch.float64)
    w = fw[0]
    y = iv @ (fw @ x)
    assert torch.allclose(y, x * w * w, atol=1e-5)


def test_library_exports_the_new_symbols():
    from gsv import _lib, build
    build.build(verbose=False)
    l = _lib.lib()
    for n in ("gsv_bwe_create", "gsv_bwe_destroy", "gsv_bwe_load_tensor", "gsv_bwe_finalize", "gsv_bwe_out_len", "gsv_bwe_forward",
              "gsv_bwe_debug_tensor", "gsv_postprocess_f32"):
        assert hasattr(l, n) and n in _lib.EXPORTS
