"""CPU: TTS.plan_cfm -- which v3 / v4 folds run_batch(shared_cfm=True) shares, how a fold is cut into rows and where a
pass ends -- and the C ABI of the rows entry.  No compute is called here."""
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from gsv.TTS_infer_pack.TTS import TTS

VC = {"T_ref": 20, "T_chunk": 48, "overlapped_len": 4, "upsample_rate": 256, "sr": 24000}


def _stub(max_rows, use_vocoder=True, vc=VC):
    return SimpleNamespace(configs=SimpleNamespace(use_vocoder=use_vocoder), vocoder_configs=dict(vc), cfm_max_rows=max_rows,
                           _chunk_cuts=TTS._chunk_cuts)


def _plan(T_min, folds, **opts):
    return dict(T_min=T_min, cfm_folds=list(folds), opts=TTS._request_options(opts))


def _reference_cuts(frames, chunk_len, ov):
    """the slicing loop that using_vocoder_synthesis_batched_infer ran inline before _chunk_cuts took its place (see the
    git history of gsv/TTS_infer_pack/TTS.py), on a tensor whose values are their own positions -> per chunk (first
    position, frames taken, padding)"""
    padded = F.pad(torch.arange(1, frames + 1, dtype=torch.float32).view(1, 1, -1), (ov, 0))
    pos_axis = torch.arange(padded.shape[2]).view(1, 1, -1)
    chunks, pos = [], 0
    while True:
        if pos != 0:
            pos -= ov
        chunk = pos_axis[:, :, pos:pos + chunk_len]
        pos += chunk_len
        if chunk.shape[-1] == 0:
            break
        chunks.append((int(chunk[0, 0, 0]), int(chunk.shape[2]), chunk_len - int(chunk.shape[2])))
    return chunks


def test_keyword_and_class_attribute():
    assert inspect.signature(TTS.run_batch).parameters["shared_cfm"].default is False
    assert inspect.signature(TTS.run_batch).parameters["shared_sovits"].default is False
    assert isinstance(TTS.cfm_max_rows, int) and TTS.cfm_max_rows >= 1


@pytest.mark.parametrize("T_min", [14, 20])              # below and at T_ref; a longer prompt reaches here cut to T_ref (next test)
@pytest.mark.parametrize("frames", [1, 27, 28, 29, 56, 150, 333])
def test_chunk_cuts_equal_the_batched_infer_loop(T_min, frames):
    chunk_len, ov = VC["T_chunk"] - T_min, VC["overlapped_len"]
    want = _reference_cuts(frames, chunk_len, ov)
    got = TTS._chunk_cuts(frames, chunk_len, ov)
    assert [(a, b - a, chunk_len - (b - a)) for a, b in got] == want
    assert got[0][0] == 0 and got[-1][1] == frames + ov
    assert all(a1 == a0 + chunk_len - ov for (a0, _), (a1, _) in zip(got, got[1:])), "a chunk starts overlapped_len before the last one's end"
    passes = TTS.plan_cfm(_stub(10 ** 6), [_plan(T_min, [frames])])
    assert passes == [[(0, 0, k) for k in range(len(want))]]


@pytest.mark.parametrize("mel_frames,fea_frames,want", [(14, 31, 14), (33, 20, 20), (27, 31, 20)])   # below, at, above T_ref
def test_prompt_longer_than_t_ref_is_cut_before_the_chunks_are(mel_frames, fea_frames, want):
    """_prompt_features gives T_min = min(mel, fea_ref) frames and keeps the LAST T_ref of a longer prompt; the chunks of that
    voice are then cut with chunk_len = T_chunk - T_min"""
    mel = torch.arange(100 * mel_frames, dtype=torch.float32).view(1, 100, mel_frames) / 100.0
    fea = torch.arange(512 * fea_frames, dtype=torch.float32).view(1, 512, fea_frames)
    vits = SimpleNamespace(decode_encp=lambda codes, phones, spec: (fea, torch.zeros(1, 512, 1)))
    stub = SimpleNamespace(prompt_cache={"ref_mel": mel, "phones": [1, 2, 3], "prompt_semantic": torch.zeros(5, dtype=torch.long),
                                         "refer_spec": [(torch.zeros(1, 9, 4), None)]},
                           configs=SimpleNamespace(device="cpu"), vits_model=vits, vocoder_configs=dict(VC), precision=torch.float32)
    _, fea_ref, _, mel2, T_min = TTS._prompt_features(stub)
    assert T_min == want and mel2.shape[2] == fea_ref.shape[2] == want
    n = min(mel_frames, fea_frames)
    assert torch.equal(fea_ref, fea[:, :, n - want:n]), "the last T_ref frames of the common part"
    frames = 150
    passes = TTS.plan_cfm(_stub(10 ** 6), [_plan(T_min, [frames])])
    assert passes == [[(0, 0, k) for k in range(len(_reference_cuts(frames, VC["T_chunk"] - want, VC["overlapped_len"])))]]


def test_what_is_shared_grouping_and_caps():
    plans = [_plan(14, [150, 40]),                         # two to_batch batches: two folds, chunk_len 34
             _plan(20, [60], parallel_infer=False),        # the chunk-by-chunk path: not shared
             _plan(20, [0, 90], speed_factor=1.25),        # an empty fold is left out; speed does not matter
             _plan(17, [100], sample_steps=8),             # its own group
             _plan(20, [])]                                # no text
    n = lambda T_min, frames: len(_reference_cuts(frames, VC["T_chunk"] - T_min, VC["overlapped_len"]))
    rows32 = [(0, 0, k) for k in range(n(14, 150))] + [(0, 1, k) for k in range(n(14, 40))] + [(2, 1, k) for k in range(n(20, 90))]
    rows8 = [(3, 0, k) for k in range(n(17, 100))]
    assert TTS.plan_cfm(_stub(10 ** 6), plans) == [rows32, rows8]
    # a cap that holds the 32-step group exactly, then one below: one pass more, and fold (0, 0) or a later one spans two passes
    total = len(rows32)
    assert TTS.plan_cfm(_stub(total), plans) == [rows32] + [rows8[i:i + total] for i in range(0, len(rows8), total)]
    cut = TTS.plan_cfm(_stub(total - 1), plans)
    assert cut[0] == rows32[:total - 1] and cut[1] == rows32[total - 1:]
    assert len(cut) == len(TTS.plan_cfm(_stub(total), plans)) + 1
    # a cap inside the first fold: it spans two passes, nothing is lost or doubled
    small = TTS.plan_cfm(_stub(3), plans)
    assert small[0] == rows32[:3] and small[1][0] == (0, 0, 3)
    assert all(1 <= len(p) <= 3 for p in small)
    flat = [e for p in small for e in p]
    assert flat == rows32 + rows8
    # every pass is of one sample_steps group
    for p in small:
        assert len({plans[r]["opts"]["sample_steps"] for r, _, _ in p}) == 1


def test_voice_key_is_by_content_not_by_dict():
    """two voice dicts holding the same stored objects are one voice for both shared stages; another prompt mel is another
    voice for the flow-matching stage only"""
    spec, sem, phones, mel = [(torch.zeros(1, 9, 4), None)], torch.zeros(5, dtype=torch.long), [1, 2, 3], torch.zeros(1, 100, 30)
    a = {"refer_spec": spec, "prompt_semantic": sem, "phones": phones, "ref_mel": mel, "sv_emb": None}
    b, c = dict(a), dict(a, ref_mel=torch.zeros(1, 100, 31))
    for fields in (("refer_spec", "sv_emb"), TTS._CFM_VOICE_FIELDS):
        assert TTS._voice_key(a, fields) == TTS._voice_key(b, fields)
    assert TTS._voice_key(a) == TTS._voice_key(c)
    assert TTS._voice_key(a, TTS._CFM_VOICE_FIELDS) != TTS._voice_key(c, TTS._CFM_VOICE_FIELDS)


def test_v2_shares_nothing():
    assert TTS.plan_cfm(_stub(32, use_vocoder=False), [_plan(14, [150]), _plan(20, [70])]) == []


def test_library_exports_the_rows_entry_and_the_header_declares_it():
    from gsv import build, _lib
    build.build(verbose=False)
    assert hasattr(_lib.lib(), "gsv_cfm_inference_rows")
    assert "gsv_cfm_inference_rows" in _lib.EXPORTS
    src = open(os.path.join(ROOT, "include", "gsv.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+gsv_cfm_inference_rows\s*\(", src)
