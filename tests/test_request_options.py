"""CPU: the single owners of the request pipeline's small facts -- the option resolver against a table written out from the
rules run() had inline, the token-keeping helper, CFM.row_seed, and that TTS.py holds no second copy of them."""
import inspect
from types import SimpleNamespace

import pytest
import torch

from gsv.module.models import CFM
from gsv.TTS_infer_pack import TTS as tts_module
from gsv.TTS_infer_pack.TTS import TTS

DEFAULTS = dict(top_k=5, top_p=1, temperature=1, batch_size=1, batch_threshold=0.75, speed_factor=1.0, split_bucket=True,
                return_fragment=False, fragment_interval=0.3, seed=-1, parallel_infer=True, repetition_penalty=1.35,
                sample_steps=32, inference_cfg_rate=0, super_sampling=False)

# (version, request, what differs from DEFAULTS once resolved)
TABLE = [
    ("v2", {}, {}),
    ("v2", {"seed": ""}, {}),
    ("v2", {"seed": None}, {}),
    ("v2", {"seed": 7}, {"seed": 7}),
    ("v2", {"fragment_interval": 0.001}, {"fragment_interval": 0.01}),
    ("v2", {"return_fragment": True, "split_bucket": True}, {"return_fragment": True, "split_bucket": False}),
    ("v2", {"speed_factor": 1.25}, {"speed_factor": 1.25, "split_bucket": False}),
    ("v3", {"parallel_infer": True}, {"split_bucket": False}),
    ("v3", {"parallel_infer": False}, {"parallel_infer": False}),
    ("v2", {"super_sampling": True}, {}),
    ("v3", {"super_sampling": True}, {"super_sampling": True, "split_bucket": False}),
    ("v4", {"super_sampling": True}, {"split_bucket": False}),
    ("v4", {"super_sampling": True, "parallel_infer": False}, {"parallel_infer": False}),
]


def _stub(version):
    return SimpleNamespace(configs=SimpleNamespace(version=version, use_vocoder=version in ("v3", "v4")),
                           _request_options=TTS._request_options)


@pytest.mark.parametrize("version,req,diff", TABLE, ids=[f"{v}-{sorted(r.items())}" for v, r, _ in TABLE])
def test_resolved_options_against_the_table(version, req, diff):
    got = TTS._resolve_options(_stub(version), dict(req))
    assert got == dict(DEFAULTS, **diff)
    assert all(type(got[k]) is type(v) for k, v in dict(DEFAULTS, **diff).items())


def test_kept_tokens():
    rows = [torch.arange(5), torch.arange(0), torch.arange(3)]
    pred, idx_list = TTS._kept_tokens(rows, [0, 0, 0], True)        # prompt-free: idx is reported as 0, everything is kept
    assert idx_list == [5, 0, 3] and all(torch.equal(a, b) for a, b in zip(pred, rows))
    rows = [torch.arange(10), torch.arange(10, 18), torch.arange(20, 24)]
    pred, idx_list = TTS._kept_tokens(rows, [4, 0, 1], False)       # with a prompt: the last idx tokens, none for idx == 0
    assert idx_list == [4, 0, 1]
    assert [p.tolist() for p in pred] == [[6, 7, 8, 9], [], [23]]


@pytest.mark.parametrize("s", [0, 5, 2 ** 63, 2 ** 64 - 1])
@pytest.mark.parametrize("b", [0, 1, 31])
def test_row_seed(s, b):
    assert CFM.row_seed(s, b) == (s + 0x9E3779B97F4A7C15 * b) & (2 ** 64 - 1)


def test_single_owners_in_the_source():
    assert "inputs.get(" not in inspect.getsource(TTS.run), "run() reads its options from _resolve_options"
    assert "9e3779b97f4a7c15" not in inspect.getsource(tts_module).lower(), "the row noise key is CFM.row_seed's"
