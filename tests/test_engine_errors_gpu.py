"""GPU: what the five engine handles share (gsveng::Ctx, csrc/engine.h) as seen through the C ABI -- a finalize that finds a
tensor missing names the tensor under the engine's own prefix, leaves nothing behind that a destroy does not release, and a
finalized handle refuses further tensors.  Nothing is launched: the handles are created from the small synthetic configs of
the engines' own GPU tests and never run."""
import ctypes as C
import json
import re

import pytest
import torch

from conftest import load_golden
from gsv import _lib, synthetic as S
from oracle import cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _Handle:
    """an engine handle created through the C ABI alone (AP_BWE has no unloaded state)"""

    def __init__(self, h):
        self._h = h


def _t2s():
    from gsv.AR.models.t2s_model import Text2SemanticDecoder
    cfg, sd = cases.t2s_case_inputs(cases.T2S_CASES["t2s_small_greedy"])[:2]

    def empty():
        return Text2SemanticDecoder(cfg, device=DEV, dtype=torch.float32, max_batch=8, max_seq=256)
    return empty, lambda: empty().load_state_dict(sd)


def _vits():
    from gsv.module.models import SynthesizerTrn
    cfg, sd = cases.vits_case_inputs(cases.VITS_CASES["vits_small"])[:2]
    d, mk = cfg["data"], dict(cfg["model"])
    version = mk.pop("version", "v2")

    def empty():
        return SynthesizerTrn(d["filter_length"] // 2 + 1, cfg["train"]["segment_size"] // d["hop_length"],
                              n_speakers=d["n_speakers"], version=version, device=DEV, dtype=torch.float32,
                              n_symbols=cfg["n_symbols"], **mk)
    return empty, lambda: empty().load_state_dict(sd)


def _vocoder():
    from gsv.BigVGAN.bigvgan import BigVGAN
    cfg = S.small_vocoder_config("bigvgan")
    sd = S.make_vocoder_state_dict(cfg, seed=11)

    def empty():
        return BigVGAN({k: v for k, v in cfg.items() if k != "kind"}, device=DEV, dtype=torch.float32)._e   # holds the handle
    return empty, lambda: empty().load_state_dict(sd)


def _cfm():
    from gsv.f5_tts.model.backbones.dit import DiT
    cfg, sd = cases.cfm_case_inputs(cases.CFM_CASES["cfm_small"])[:2]

    def empty():
        return DiT(dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], dim_head=cfg["dim_head"], ff_mult=cfg["ff_mult"],
                   mel_dim=cfg["mel_dim"], text_dim=cfg["text_dim"], conv_layers=cfg["conv_layers"], device=DEV, dtype=torch.float32)
    return empty, lambda: empty().load_state_dict(sd)


def _bwe():
    from gsv.tools.audio_sr import AP_BWE
    g = load_golden("bwe_small")
    cfg = json.loads(str(g["config"]))

    def empty():
        c = _lib.BweConfig()
        c.n_fft, c.hop_size, c.win_size = cfg["n_fft"], cfg["hop_size"], cfg["win_size"]
        c.channels, c.layers, c.hr_sampling_rate = cfg["ConvNeXt_channels"], cfg["ConvNeXt_layers"], cfg["hr_sampling_rate"]
        h = C.c_void_p()
        with torch.cuda.device(DEV):
            _lib.init(0)
            _lib.check(_lib.lib().gsv_bwe_create(C.byref(c), _lib.GSV_F32, C.byref(h)), "gsv_bwe_create")
        return _Handle(h)
    return empty, lambda: AP_BWE(DEV, state={"generator": S.make_bwe_state_dict(cfg, int(g["seed"]))}, config=cfg)


ENGINES = {"t2s": _t2s, "vits": _vits, "vocoder": _vocoder, "cfm": _cfm, "bwe": _bwe}


def _library_message(exc):
    """the library's own message inside _lib.check's RuntimeError ("libgsv_hip <what> failed (rc=N): <message>")"""
    m = re.fullmatch(r"libgsv_hip .* failed \(rc=-?\d+\): (.*)", str(exc), re.S)
    assert m, str(exc)
    return m.group(1)


@pytest.mark.parametrize("who", list(ENGINES))
def test_failed_finalize_names_engine_and_tensor_and_finalized_handle_refuses_tensors(who):
    l = _lib.lib()
    fn = {k: getattr(l, f"gsv_{who}_{k}") for k in ("finalize", "destroy", "load_tensor")}
    empty, good = ENGINES[who]()
    with torch.cuda.device(DEV):
        # finalize with nothing loaded: the first tensor the engine asks for, under the engine's own prefix
        bad = empty()
        with pytest.raises(RuntimeError) as e:
            _lib.check(fn["finalize"](bad._h), f"gsv_{who}_finalize")
        msg = _library_message(e.value)
        print(msg)
        assert msg.startswith(f"{who}: "), msg
        assert re.search(r"tensor '[\w.]+'", msg), msg
        fn["destroy"](bad._h)
        bad._h = None
        # the failed finalize left nothing behind: a fresh handle of the same shape loads and finalizes
        eng = good()
        # ... and is closed to further tensors
        t = torch.zeros(4)
        with pytest.raises(RuntimeError) as e:
            _lib.check(fn["load_tensor"](eng._h, b"late.weight", t.data_ptr(), t.numel()), "load late.weight")
        assert "already finalized" in _library_message(e.value), str(e.value)
