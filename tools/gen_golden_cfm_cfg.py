"""TEST INFRASTRUCTURE ONLY -- golden vectors for classifier-free guidance in the v3/v4 flow-matching decoder: the REFERENCE
`CFM.inference(..., inference_cfg_rate=r)` (module/models.py:1027-1085; needs the reference checkout that oracle/ref_import.py
reaches) at r = 0.7 and 2.0 on the `cfm_small` and `cfm_v3dims` cases of oracle/cases.py, with `torch.randn`
pinned as oracle/gen_golden_vits.py::gen_cfm pins it.  Asserts that tests/_cfg_ref.py restates the same loop within gen_cfm's
bar (2e-4 max-abs) and writes tests/golden/<case>_cfg.npz with one array per rate."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "gpt-sovits_amd"), ROOT):
    sys.path.insert(0, p)

from oracle import ref_import  # noqa: E402
from oracle.cases import CFM_CASES, cfm_case_inputs  # noqa: E402
import _cfg_ref  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = ("cfm_small", "cfm_v3dims")


def main():
    ref_import.setup()
    from GPT_SoVITS.f5_tts.model.backbones.dit import DiT
    from module.models import CFM
    for name in NAMES:
        case = CFM_CASES[name]
        cfg, sd, mu, prompt, noise = cfm_case_inputs(case)
        dit = DiT(dim=cfg["dim"], depth=cfg["depth"], heads=cfg["heads"], dim_head=cfg["dim_head"], ff_mult=cfg["ff_mult"],
                  mel_dim=cfg["mel_dim"], text_dim=cfg["text_dim"], conv_layers=cfg["conv_layers"])
        dit.load_state_dict(sd, strict=True)
        cfm = CFM(cfg["mel_dim"], dit).eval()
        lens = torch.LongTensor([case["T"]] * case["B"])
        out = {}
        orig = torch.randn
        torch.randn = lambda *a, **k: noise.clone()
        try:
            plain = cfm.inference(mu, lens, prompt, case["steps"], inference_cfg_rate=0)
            for rate in _cfg_ref.RATES:
                out[rate] = cfm.inference(mu, lens, prompt, case["steps"], inference_cfg_rate=rate)
        finally:
            torch.randn = orig
        for rate, ref in out.items():
            mine = _cfg_ref.cfm_inference_cfg(sd, cfg, mu, prompt, case["steps"], noise.clone(), rate)
            err = (mine - ref).abs().max().item()
            moved = (ref - plain).abs().max().item()
            print(f"[gen_golden_cfm_cfg] {name} r = {rate}: out {tuple(ref.shape)} absmax {ref.abs().max():.3f} "
                  f"helper max-abs err {err:.2e}, guided - unguided max-abs {moved:.2f}")
            assert err <= 2e-4
        np.savez_compressed(os.path.join(GOLD, name + "_cfg.npz"),
                            **{_cfg_ref.golden_key(r): v.numpy().astype(np.float32) for r, v in out.items()})


if __name__ == "__main__":
    main()
