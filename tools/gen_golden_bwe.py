"""TEST INFRASTRUCTURE ONLY -- fixtures of the AP-BWE super-sampling path, produced by the REFERENCE's own classes (build
container only; the reference tree does not travel to the GPU machine):

  tests/golden/bwe_small.npz   every stage of tools/audio_sr.py::AP_BWE.__call__ (resampled, log_amp, pha, mag_wb, pha_wb,
                               output) at a reduced config, 24 kHz input with an all-zero stretch; the output of a 32 kHz input
  tests/golden/bwe_full.npz    0.25 s of 24 kHz input end to end at the assumed published 24k -> 48k shape, and 0.125 s of
                               full-band 48 kHz input (both fixtures)
  tests/golden/bwe_glue.npz    TTS.audio_postprocess(..., super_sampling=True) (TTS.py:1377-1429) on
                               gsv.synthetic.make_bwe_fragments, called unbound with sr_model = the reference AP_BWE at the
                               reduced config

Both fixtures also record the key set and shapes of the reference's APNet_BWE_Model state dict at their config, which the
CPU tests compare against gsv.synthetic.make_bwe_state_dict.  torchaudio is absent: `torchaudio.functional.resample` is the
restatement gsv.tools.audio_sr.resample ("parity unpinned" against the package itself).  Weights are gsv.synthetic hash
weights; only seeds, shapes and outputs are committed.

One backend detail is normalised: on an all-zero frame (the fragment_interval gaps), the CPU FFT behind torch.stft returns
-0 real parts in the upper half of the bins, and torch.angle(-0 + 0j) is pi there, while an exact-zero bin is +0 with phase 0
on other backends.  The phase of an exact-zero bin is 0 in the engine; here torch.stft's result gets +0 added (which turns
-0 into +0 and changes nothing else), so that the fixtures hold the reference's model output for that same input.  The
inputs start and end with exact zeros for the same reason (gsv.synthetic.make_bwe_input).

    python tools/gen_golden_bwe.py
"""
import importlib.util
import json
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gpt-sovits_amd"))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")

from gsv import synthetic as S  # noqa: E402
from gsv.tools.audio_sr import resample  # noqa: E402
from oracle import ref_import  # noqa: E402

SEED = 0


def inputs_small():
    """0.1 s at 24 kHz with 0.03 s of exact zeros in the middle (all-zero STFT frames), and 0.1 s at 32 kHz"""
    return S.make_bwe_input("bwe_in_small", 2400, gap=(900, 1620)), S.make_bwe_input("bwe_in_32k", 3200, lead=400, tail=400)


def input_full():
    return S.make_bwe_input("bwe_in_full", 6000)


def input_48k():
    """0.125 s of full-band noise at 48 kHz (no resampling): every bin carries signal, so the log-amplitude and the phase
    fed to the model are well conditioned (see tests/test_audio_sr_gpu.py)"""
    return S.make_bwe_input("bwe_in_48k", 6000, lead=600, tail=600)


class _Attr(dict):
    def __getattr__(self, k):
        return self[k]


def ref_ap_bwe(cfg, sd):
    """the reference's AP_BWE built from a config.json + torch.save({"generator": sd}) in a temp dir"""
    spec = importlib.util.spec_from_file_location("ref_audio_sr", os.path.join(ref_import.REF_ROOT, "tools", "audio_sr.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    d = tempfile.mkdtemp()
    with open(os.path.join(d, "config.json"), "w") as f:
        json.dump(cfg, f)
    torch.save({"generator": sd}, os.path.join(d, "g.pt"))
    return mod.AP_BWE("cpu", _Attr, checkpoint_file=os.path.join(d, "g.pt")), mod


def schema(model):
    return np.array(json.dumps({k: list(v.shape) for k, v in model.state_dict().items()}))


def main():
    RT = ref_import.tts_module()
    ta = sys.modules["torchaudio"]
    ta.functional = ref_import._stub("torchaudio.functional", resample=resample)
    torch.set_num_threads(8)
    stft = torch.stft

    def stft_pos0(*a, **k):
        X = stft(*a, **k)
        return torch.complex(X.real + 0.0, X.imag + 0.0)

    torch.stft = stft_pos0
    sys.path.append(os.path.join(ref_import.REF_ROOT, "tools", "AP_BWE_main"))
    from datasets1.dataset import amp_pha_stft  # noqa: E402

    # ---- reduced config: every stage
    cfg = S.small_bwe_config()
    sr_model, _ = ref_ap_bwe(cfg, S.make_bwe_state_dict(cfg, SEED))
    h = sr_model.h
    x24, x32 = inputs_small()
    out = {"seed": np.array(SEED), "config": np.array(json.dumps(cfg)), "sd_schema": schema(sr_model.model)}
    with torch.no_grad():
        y = resample(x24, 24000, h.hr_sampling_rate)
        la, pha, _ = amp_pha_stft(y, h.n_fft, h.hop_size, h.win_size)
        mag_wb, pha_wb, _ = sr_model.model(la, pha)
    wav, sr = sr_model(x24, 24000)
    assert sr == 48000
    out.update(resampled=y[0].numpy(), log_amp=la[0].numpy(), pha=pha[0].numpy(), mag_wb=mag_wb[0].numpy(), pha_wb=pha_wb[0].numpy(),
               out=wav.astype(np.float32))
    wav32, _ = sr_model(x32, 32000)
    out["out_32k"] = wav32.astype(np.float32)
    out["out_48k"] = sr_model(input_48k(), 48000)[0].astype(np.float32)
    np.savez_compressed(os.path.join(GOLD, "bwe_small.npz"), **out)
    zf = int((np.abs(pha[0].numpy()).max(0) == 0).sum())
    print(f"[gen_golden] bwe_small: {wav.shape[0]} samples, {la.shape[-1]} frames ({zf} all-zero), 32k -> {wav32.shape[0]}")

    # ---- assumed published shape: end to end
    fcfg = dict(S.BWE_24K_48K_CONFIG)
    full, _ = ref_ap_bwe(fcfg, S.make_bwe_state_dict(fcfg, SEED))
    wav, _ = full(input_full(), 24000)
    np.savez_compressed(os.path.join(GOLD, "bwe_full.npz"), seed=np.array(SEED), config=np.array(json.dumps(fcfg)),
                        sd_schema=schema(full.model), out=wav.astype(np.float32),
                        out_48k=full(input_48k(), 48000)[0].astype(np.float32))
    print(f"[gen_golden] bwe_full: {wav.shape[0]} samples, rms {np.sqrt((wav ** 2).mean()):.4f}")

    # ---- TTS.audio_postprocess(super_sampling=True) with the reference AP_BWE bound as sr_model
    ns = SimpleNamespace(configs=SimpleNamespace(device="cpu", sampling_rate=32000), precision=torch.float32,
                         sr_model=sr_model, sr_model_not_exist=False)
    ns.recovery_order = lambda data, bil: RT.TTS.recovery_order(ns, data, bil)
    ns.init_sr_model = lambda: None
    glue = {}
    for sr_in in (24000, 48000):              # 48000: full-band fragments, no resampling (well conditioned)
        for sb in (True, False):
            audio, bil = S.make_bwe_fragments(torch.float32)
            sr, a16 = RT.TTS.audio_postprocess(ns, audio, sr_in, bil, 1.0, sb, 0.3, True)
            assert sr == 48000 and a16.dtype == np.int16
            glue[f"post{sr_in // 1000}k_{'bucket' if sb else 'flat'}"] = a16
    np.savez_compressed(os.path.join(GOLD, "bwe_glue.npz"), **glue)
    print(f"[gen_golden] bwe_glue: {glue['post24k_bucket'].shape[0]} samples")


if __name__ == "__main__":
    main()
