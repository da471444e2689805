"""CPU: tests/_cfg_ref.py -- the restated `CFM.inference(..., inference_cfg_rate=r)` that the guided GPU tests compare
against -- held to goldens written by the reference class itself (tools/gen_golden_cfm_cfg.py), at the bar
oracle/gen_golden_vits.py::gen_cfm sets for the unguided oracle: 2e-4 max-abs."""
import numpy as np
import pytest
import torch

import _cfg_ref
from conftest import load_golden
from oracle import cases, cfm_oracle

NAMES = ("cfm_small", "cfm_v3dims")


@pytest.mark.parametrize("rate", _cfg_ref.RATES)
@pytest.mark.parametrize("name", NAMES)
def test_helper_matches_the_reference_class(name, rate):
    case = cases.CFM_CASES[name]
    cfg, sd, mu, prompt, noise = cases.cfm_case_inputs(case)
    g = load_golden(name + "_cfg")[_cfg_ref.golden_key(rate)]
    out = _cfg_ref.cfm_inference_cfg(sd, cfg, mu, prompt, case["steps"], noise.clone(), rate).numpy()
    assert out.shape == g.shape
    err = float(np.abs(out - g).max())
    print(f"[parity] {name} r = {rate}: helper vs reference class max-abs {err:.2e}")
    assert err <= 2e-4
    assert np.all(out[:, :, :case["Tp"]] == 0)
    # the guided golden is not the unguided one: a dropped rate cannot pass
    assert float(np.abs(g - load_golden(name)["mel"]).max()) > 1.0


@pytest.mark.parametrize("rate", [0, 1e-6, 1e-5, -0.5])
def test_rate_at_or_below_the_threshold_is_the_unguided_oracle(rate):
    """guidance is active iff rate > 1e-5 (models.py:1063): zero, tiny and negative rates are cfm_oracle.cfm_inference"""
    case = cases.CFM_CASES["cfm_small"]
    cfg, sd, mu, prompt, noise = cases.cfm_case_inputs(case)
    out = _cfg_ref.cfm_inference_cfg(sd, cfg, mu, prompt, case["steps"], noise.clone(), rate)
    assert torch.equal(out, cfm_oracle.cfm_inference(sd, cfg, mu, prompt, case["steps"], noise.clone()))
