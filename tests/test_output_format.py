"""CPU: the request keys "sample_rate" and "encoding"  on their way to the kernel -- validation and the
only-when-given rule of the option resolver, the supported-pair predicate, the wire formats and the sharding refusal."""
import struct
from io import BytesIO
from types import SimpleNamespace

import numpy as np
import pytest

from gsv import audio_io, sharding, wire
from gsv.TTS_infer_pack.TTS import TTS

MODEL_RATES = [24000, 32000, 48000]
OUT_RATES = [8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000]


def _stub(version="v2", sr=32000, calls=None):
    def output_sr():
        if calls is not None:
            calls.append(1)
        return sr
    return SimpleNamespace(configs=SimpleNamespace(version=version, use_vocoder=version in ("v3", "v4")),
                           _request_options=TTS._request_options, _output_sr=output_sr)


def test_keys_are_carried_only_when_given():
    base = TTS._request_options({})
    assert "sample_rate" not in base and "encoding" not in base
    assert TTS._request_options({"sample_rate": None, "encoding": None}) == base
    assert TTS._request_options({"sample_rate": 8000}) == dict(base, sample_rate=8000)
    assert TTS._request_options({"encoding": "mulaw"}) == dict(base, encoding="mulaw")
    assert TTS._format_kw(base) == {}
    assert TTS._format_kw(dict(base, sample_rate=8000, encoding="alaw")) == {"sample_rate": 8000, "encoding": "alaw"}


@pytest.mark.parametrize("req", [{"sample_rate": 0}, {"sample_rate": -8000}, {"sample_rate": 8000.0}, {"sample_rate": "8000"},
                                 {"sample_rate": True}, {"encoding": "pcm_u8"}, {"encoding": "MULAW"}, {"encoding": 1}])
def test_bad_values_raise_before_any_stage(req):
    with pytest.raises(ValueError):
        TTS._request_options(req)
    with pytest.raises(ValueError):
        TTS._resolve_options(_stub(), dict(req))


def test_resolution_drops_what_the_default_path_gives_anyway():
    calls = []
    base = TTS._resolve_options(_stub(calls=calls), {})
    assert calls == [], "_output_sr() is asked only when the request names a rate"
    assert TTS._resolve_options(_stub(calls=calls), {"encoding": "mulaw"}) == dict(base, encoding="mulaw") and calls == []
    assert TTS._resolve_options(_stub(calls=calls), {"sample_rate": 32000, "encoding": "pcm_s16"}) == base
    assert calls == [1]
    assert TTS._resolve_options(_stub("v3", 24000), {"sample_rate": 24000, "parallel_infer": False}) == dict(base, parallel_infer=False)
    got = TTS._resolve_options(_stub(), {"sample_rate": 8000, "encoding": "alaw"})
    assert got == dict(base, sample_rate=8000, encoding="alaw")
    got = TTS._resolve_options(_stub(), {"sample_rate": 32000, "encoding": "mulaw"})
    assert got == dict(base, encoding="mulaw")


def test_an_unsupported_pair_is_refused_in_the_resolver():
    with pytest.raises(ValueError, match="32000 -> 50"):
        TTS._resolve_options(_stub(), {"sample_rate": 50})              # 640 inputs per output: a window far past the kernel's LDS
    with pytest.raises(ValueError):
        TTS._resolve_options(_stub(sr=32000), {"sample_rate": 44101})   # coprime rates: a filter of 640 k taps


@pytest.mark.parametrize("sr_in", MODEL_RATES)
def test_supported_pairs(sr_in):
    pairs = [(sr_in, r) for r in OUT_RATES if r != sr_in]
    assert len(pairs) == 7                                              # 21 pairs over the three model rates
    for a, b in pairs:
        assert audio_io.output_rate_supported(a, b), (a, b)
        h, up, down = audio_io.output_filter(a, b)
        win = (1023 * down + len(h) - 1) // up + 2
        assert win <= 6260 and len(h) % 2 == 1
        in_lds = max(win, 1024) + len(h) <= audio_io.RS_LDS_FLOATS
        assert in_lds == ((a, b) not in [(32000, 11025), (48000, 11025)])   # these two read their filters through L2
    assert audio_io.output_rate_supported(sr_in, sr_in)
    h, up, down = audio_io.output_filter(sr_in, sr_in)
    assert h.tolist() == [1.0] and h.dtype == np.float32 and (up, down) == (1, 1)
    assert not audio_io.output_rate_supported(sr_in, 0) and not audio_io.output_rate_supported(sr_in, 50)
    assert audio_io.ENCODINGS == {"pcm_s16": 0, "mulaw": 1, "alaw": 2}


class _Pipeline:
    """what tts_handle needs of a pipeline: run(req) yields (sr, audio) in the format the request names"""

    def __init__(self):
        self.seen = []

    def run(self, req):
        self.seen.append(req)
        sr = req.get("sample_rate", 32000)
        n = 3 if req.get("return_fragment") else 1
        for i in range(n):
            if req.get("encoding") in ("mulaw", "alaw"):
                yield sr, np.arange(5 + i, dtype=np.uint8)
            else:
                yield sr, np.arange(5 + i, dtype=np.int16)


def test_wire_carries_the_rate_and_the_bytes():
    p = _Pipeline()
    code, mt, body = wire.tts_handle(p, {"text": "x", "sample_rate": 8000})
    assert code == 200 and mt == "audio/wav" and struct.unpack("<I", body[24:28])[0] == 8000 and len(body) == 44 + 10
    code, mt, body = wire.tts_handle(p, {"text": "x", "sample_rate": 8000, "encoding": "mulaw", "media_type": "raw"})
    assert code == 200 and mt == "audio/raw" and body == bytes(range(5))
    assert wire.pack_raw(BytesIO(), np.array([0xff, 0x80, 0x00], dtype=np.uint8), 8000).getvalue() == b"\xff\x80\x00"
    code, mt, chunks = wire.tts_handle(p, {"text": "x", "sample_rate": 16000, "streaming_mode": True})
    chunks = list(chunks)
    assert code == 200 and struct.unpack("<I", chunks[0][24:28])[0] == 16000 and len(chunks) == 4


@pytest.mark.parametrize("media_type", ["wav", "aac", "ogg"])
@pytest.mark.parametrize("enc", ["mulaw", "alaw"])
def test_g711_in_a_pcm_container_is_a_400(media_type, enc):
    p = _Pipeline()
    code, mt, body = wire.tts_handle(p, {"text": "x", "encoding": enc, "media_type": media_type})
    assert code == 400 and mt == "application/json" and "raw" in body["Exception"] and p.seen == []
    with pytest.raises(ValueError):
        wire.pack_audio(BytesIO(), np.zeros(4, dtype=np.uint8), 8000, media_type)
    code, _, _ = wire.tts_handle(p, {"text": "x", "encoding": enc})                  # media_type defaults to wav
    assert code == 400


@pytest.mark.parametrize("key,value", [("sample_rate", 16000), ("encoding", "mulaw")])
def test_sharding_refuses_the_keys(key, value):
    seg = {"phones": [1, 2, 3], "norm_text": "abc", key: value}
    with pytest.raises(ValueError, match=key):
        sharding.refuse_output_format([seg])
    sharding.refuse_output_format([{"phones": [1], "norm_text": "a"}])
    sharding.refuse_output_format(None)
    import torch
    synth = sharding.ShardedSynthesizer(lambda segs: (_ for _ in ()).throw(AssertionError("the engine ran")), torch.device("cpu"))
    with pytest.raises(ValueError, match=key):
        synth.run([seg], batch_size=1)
    with pytest.raises(ValueError, match=key):
        list(synth.run_stream([seg], batch_size=1))
