"""GPU: SV.compute_embedding3_many / ERes2NetV2.forward3_segments, the packed speaker-embedding pass, against
oracle.sv_oracle.compute_embedding3 per audio, at the bars of test_eres2netv2_embedding_matches_reference (relative rms <= 1e-4,
max-abs <= 2e-3).  Full-size synthetic weights; audios of 1737, 2800, 4079 and 16410 samples = 9, 16, 23 and 101 fbank frames
(remainders 57, 0, 79, 10 below the next frame): a frame count that is a multiple of 8, odd lengths at every stride level
(9 -> 5 -> 3 -> 2; 23 -> 12 -> 6 -> 3; 101 -> 51 -> 26 -> 13), a segment two rows long at T / 8."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LENS = [1737, 2800, 4079, 16410]


@pytest.fixture(scope="module")
def world():
    from gsv import synthetic as S
    from gsv.sv import SV
    from oracle import sv_oracle as so
    sd = S.make_eres2net_state_dict(seed=0)
    wavs = [S.make_waveform(n, 20 + i) for i, n in enumerate(LENS)]
    refs = [so.compute_embedding3(sd, w.unsqueeze(0))[0].numpy() for w in wavs]
    assert all(np.isfinite(r).all() and r.shape == (20480,) for r in refs)
    return dict(sd=sd, sv=SV(DEV, False, state_dict=sd), wavs=wavs, refs=refs)


def _check(tag, emb, ref):
    assert tuple(emb.shape) == (1, 20480) and emb.dtype == torch.float32
    o = emb[0].cpu().numpy()
    rel, err = np.sqrt(((o - ref) ** 2).mean() / (ref ** 2).mean()), np.abs(o - ref).max()
    print(f"[sv segments] {tag}: relative rms {rel:.2e}, max-abs {err:.2e}")
    assert rel <= 1e-4 and err <= 2e-3


def test_packed_pass_matches_oracle_per_audio(world):
    sv, net = world["sv"], world["sv"].embedding_model
    p0, o0 = net.seg_passes, net.one_passes
    embs = sv.compute_embedding3_many([w.to(DEV) for w in world["wavs"]])
    assert net.seg_passes == p0 + 1 and net.one_passes == o0 and len(embs) == 4
    for n, e, r in zip(LENS, embs, world["refs"]):
        _check(f"{n} samples, one pass", e, r)


def test_several_passes_and_reversed_order(world):
    sv, net = world["sv"], world["sv"].embedding_model
    p0 = net.seg_passes
    embs = sv.compute_embedding3_many([w.unsqueeze(0) for w in world["wavs"]], max_frames=64)      # slots 24 + 24 | 32 | 112
    assert net.seg_passes == p0 + 3
    for n, e, r in zip(LENS, embs, world["refs"]):
        _check(f"{n} samples, max_frames 64", e, r)
    embs = sv.compute_embedding3_many(world["wavs"][::-1])
    for n, e, r in zip(LENS[::-1], embs, world["refs"][::-1]):
        _check(f"{n} samples, reversed", e, r)


def test_neighbours_do_not_reach_an_audio(world):
    from gsv import synthetic as S
    sv = world["sv"]
    a = sv.compute_embedding3_many(world["wavs"])
    others = [S.make_waveform(n, 70 + i) * 1.7 for i, n in enumerate(LENS[:3])] + [world["wavs"][3]]
    b = sv.compute_embedding3_many(others)
    assert torch.equal(a[3].view(torch.int32), b[3].view(torch.int32))
    assert not torch.equal(a[0], b[0])
    # and the first audio with other audios behind it
    c = sv.compute_embedding3_many([world["wavs"][0]] + others[1:3] + [S.make_waveform(LENS[3], 80)])
    assert torch.equal(a[0].view(torch.int32), c[0].view(torch.int32))


def test_launches_do_not_depend_on_the_audio_count(world):
    sv, net = world["sv"], world["sv"].embedding_model
    l0 = net.launches
    sv.compute_embedding3_many(world["wavs"][2:3])
    one = net.launches - l0
    sv.compute_embedding3_many(world["wavs"])
    four = net.launches - l0 - one
    print(f"[sv segments] launches of a packed pass: {four}")
    assert one == four > 0


def test_half_output_and_short_audio(world):
    from gsv.sv import SV
    half = SV(DEV, True, state_dict=world["sd"])
    out = half.compute_embedding3_many([w.half().to(DEV) for w in world["wavs"][:2]])
    assert [tuple(e.shape) for e in out] == [(1, 20480)] * 2 and all(e.dtype == torch.float16 for e in out)
    ref = half.compute_embedding3(world["wavs"][1].half().unsqueeze(0).to(DEV))
    rel = float((out[1].float() - ref.float()).pow(2).mean().sqrt() / ref.float().pow(2).mean().sqrt())
    assert rel <= 2e-3                                              # both are fp16 casts of fp32 results within 1e-4 of the oracle
    net = half.embedding_model
    l0, p0 = net.launches, net.seg_passes
    with pytest.raises(ValueError):
        half.compute_embedding3_many([world["wavs"][0], torch.zeros(300)])
    assert net.launches == l0 and net.seg_passes == p0
