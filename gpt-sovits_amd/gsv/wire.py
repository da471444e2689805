"""Audio wire formats and response framing of the reference's HTTP front-end (api_v2.py:176-249, 300-373): what leaves the path
as bytes, and in which pieces.

* `raw` and `wav` are byte-level formats and are built here.  `aac` is, as in the reference (api_v2.py:193-220), the output of
  an `ffmpeg` subprocess fed with s16le PCM: used when an ffmpeg executable is on PATH, refused loudly otherwise.  `ogg` needs
  libsndfile through the `soundfile` package (api_v2.py:176-179), which is not installed: refused loudly.
* `streaming_generator` is the chunked-response framing (api_v2.py:346-354): for "wav" one header-only RIFF chunk first, then
  every fragment as raw int16 bytes; other media types are packed fragment by fragment.  It consumes `TTS.run(...)` with
  `return_fragment=True` -- or `ShardedSynthesizer.run_stream` on a multi-GPU node -- and is what BASELINE configs[4] streams.
* `tts_handle` restates api_v2.py:300-373 without the web framework: request dict -> (status, media type, bytes or iterator
  of bytes); `create_app` wraps it in the reference's /tts GET / POST routes when FastAPI is importable (the HTTP server
  itself is outside the hot-path scope: this is the seam a deployment binds to)."""
from __future__ import annotations

import struct
from io import BytesIO

import numpy as np


def pack_raw(io_buffer: BytesIO, data: np.ndarray, rate: int) -> BytesIO:
    """api_v2.py:182-184: the samples' bytes as they are (int16 little endian from the path; one byte per sample, uint8, for
    a request with a G.711 "encoding")."""
    io_buffer.write(data.tobytes())
    return io_buffer


def _riff_pcm16_header(n_bytes: int, channels: int, sample_width: int, rate: int) -> bytes:
    return (b"RIFF" + struct.pack("<I", 36 + n_bytes) + b"WAVE" + b"fmt " +
            struct.pack("<IHHIIH H", 16, 1, channels, rate, rate * channels * sample_width, channels * sample_width,
                        8 * sample_width) + b"data" + struct.pack("<I", n_bytes))


def pack_wav(io_buffer: BytesIO, data: np.ndarray, rate: int) -> BytesIO:
    """api_v2.py:187-190 (`soundfile.write(..., format="wav")` of int16 mono data = canonical 44-byte RIFF/WAVE PCM_16
    header + samples).  Like the reference, a NEW buffer is returned and the one passed in is ignored.
    Parity unpinned: soundfile is not installed here, the layout is checked against the stdlib `wave` writer instead."""
    if data.dtype != np.int16:
        raise TypeError("pack_wav expects the path's int16 samples")
    out = BytesIO()
    body = np.ascontiguousarray(data).astype("<i2", copy=False).tobytes()
    out.write(_riff_pcm16_header(len(body), 1, 2, rate))
    out.write(body)
    return out


def pack_audio(io_buffer: BytesIO, data: np.ndarray, rate: int, media_type: str) -> BytesIO:
    """api_v2.py:223-233: dispatch on media type, anything unknown is raw; the buffer is rewound.  G.711 bytes (uint8: a
    request with "encoding" mulaw / alaw) leave as raw only: the containers here hold PCM."""
    if data.dtype == np.uint8 and media_type in ("wav", "aac", "ogg"):
        raise ValueError(G711_NEEDS_RAW % media_type)
    if media_type == "ogg":
        raise NotImplementedError("media_type 'ogg' needs libsndfile (the `soundfile` package, api_v2.py:176-179), which is not "
                                  "installed; request 'wav', 'raw' or 'aac'")
    if media_type == "aac":
        io_buffer = pack_aac(io_buffer, data, rate)
    elif media_type == "wav":
        io_buffer = pack_wav(io_buffer, data, rate)
    else:
        io_buffer = pack_raw(io_buffer, data, rate)
    io_buffer.seek(0)
    return io_buffer


G711_NEEDS_RAW = "media_type '%s' holds PCM: a request with encoding 'mulaw' or 'alaw' needs media_type 'raw'"


def pack_aac(io_buffer: BytesIO, data: np.ndarray, rate: int) -> BytesIO:
    """api_v2.py:193-220: ADTS AAC at 192 kb/s from an ffmpeg subprocess fed with the s16le samples."""
    import shutil
    import subprocess
    exe = shutil.which("ffmpeg")
    if exe is None:
        raise NotImplementedError("media_type 'aac' needs an `ffmpeg` executable on PATH (api_v2.py:193-220)")
    p = subprocess.Popen([exe, "-f", "s16le", "-ar", str(rate), "-ac", "1", "-i", "pipe:0", "-c:a", "aac", "-b:a", "192k", "-vn",
                          "-f", "adts", "pipe:1"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    out, _ = p.communicate(input=np.ascontiguousarray(data).tobytes())
    io_buffer.write(out)
    return io_buffer


def wave_header_chunk(frame_input: bytes = b"", channels: int = 1, sample_width: int = 2, sample_rate: int = 32000) -> bytes:
    """api_v2.py:237-249: header of a streaming wav response followed by the first frames (data length = what is known
    at that point, 0 for the bare header); later chunks are sent raw."""
    return _riff_pcm16_header(len(frame_input), channels, sample_width, sample_rate) + frame_input


def streaming_generator(tts_generator, media_type: str):
    """api_v2.py:346-354: chunked-response framing.  `tts_generator` yields (sample rate, int16 fragment)."""
    first = True
    for sr, chunk in tts_generator:
        if first and media_type == "wav":
            yield wave_header_chunk(sample_rate=sr)
            media_type = "raw"
            first = False
        yield pack_audio(BytesIO(), chunk, sr, media_type).getvalue()


def parse_timestamps(v):
    """the query-string form of the request key "timestamps": "", "0", "false", "none" are False, anything else is the mode as
    given ("sentence", "phone"; another word is refused by the pipeline)"""
    return False if str(v).strip().lower() in ("", "0", "false", "none") else str(v).strip().lower()


def tts_handle(tts_pipeline, req: dict, server=None):
    """api_v2.py:300-373 without the web framework: -> (status code, media type, payload); payload is bytes, an iterator of
    bytes (streaming_mode) or, on failure, the reference's error dict.
    server (gsv.serving.Server, e.g. tts_pipeline.serve()): the request is submitted to it and this call waits for its
    future, so that calls from several threads share the server's decode session and waveform passes.  A streaming_mode
    request goes through `server.submit_stream` where the server has it: the payload then frames each fragment when the
    scheduler emits it (a failure after the first fragment is raised by the iterator); a server without it, and a
    return_fragment request that is not streamed, hand back the list of fragments at the end."""
    streaming_mode = req.get("streaming_mode", False)
    media_type = req.get("media_type", "wav")
    if req.get("encoding") in ("mulaw", "alaw") and media_type in ("wav", "aac", "ogg"):     # before any stage runs
        return 400, "application/json", {"message": "tts failed", "Exception": G711_NEEDS_RAW % media_type}
    marked = req.get("timestamps") not in (None, False)
    if marked and (streaming_mode or req.get("return_fragment", False)):                             # before any stage runs
        return 400, "application/json", {"message": "tts failed", "Exception": "\"timestamps\" comes with the whole utterance in one "
                                         "JSON answer: not with streaming_mode / return_fragment (DESIGN.md section 4w)"}
    if streaming_mode or req.get("return_fragment", False):
        req = dict(req, return_fragment=True)
    try:
        if server is not None and streaming_mode and hasattr(server, "submit_stream"):
            gen = server.submit_stream(req)
        elif server is not None:
            result = server.submit(req).result()
            gen = iter(result if isinstance(result, list) else [result])
        else:
            gen = tts_pipeline.run(req)
        if streaming_mode:
            return 200, f"audio/{media_type}", streaming_generator(gen, media_type)
        if marked:      # speech marks: one JSON answer, the packed media as base64 beside them
            import base64
            from .timestamps import to_json
            sr, audio, marks = next(gen)
            packed = pack_audio(BytesIO(), audio, sr, media_type).getvalue()
            return 200, "application/json", {"audio": base64.b64encode(packed).decode("ascii"), "media_type": media_type,
                                             "sample_rate": int(sr), "timestamps": to_json(marks)}
        sr, audio = next(gen)
        return 200, f"audio/{media_type}", pack_audio(BytesIO(), audio, sr, media_type).getvalue()
    except Exception as e:                                              # noqa: BLE001 -- the reference answers 400 with the message
        return 400, "application/json", {"message": "tts failed", "Exception": str(e)}


def create_app(tts_pipeline, server=None):
    """the reference's /tts routes (api_v2.py:416-470) over `tts_handle`; needs fastapi (present in this image).
    server (gsv.serving.Server): every request waits for its future on a worker thread, off the event loop, so concurrent
    HTTP requests overlap in the server's decode session instead of being served one after the other."""
    import asyncio
    from fastapi import FastAPI, Request
    from fastapi.responses import JSONResponse, Response, StreamingResponse
    app = FastAPI()

    def answer(code, mt, payload):
        if code != 200:
            return JSONResponse(status_code=code, content=payload)
        if isinstance(payload, (bytes, bytearray)):
            return Response(payload, media_type=mt)
        return StreamingResponse(payload, media_type=mt)

    async def respond(req: dict):
        if server is None:
            return answer(*tts_handle(tts_pipeline, req))
        return answer(*await asyncio.get_running_loop().run_in_executor(None, tts_handle, tts_pipeline, req, server))

    async def tts_get(request):
        q = dict(request.query_params)
        for k in ("top_k", "batch_size", "seed", "sample_steps", "sample_rate"):
            if k in q:
                q[k] = int(q[k])
        for k in ("top_p", "temperature", "batch_threshold", "speed_factor", "fragment_interval", "repetition_penalty",
                  "inference_cfg_rate", "loudness", "loudness_peak"):
            if k in q:
                q[k] = float(q[k])
        for k in ("split_bucket", "streaming_mode", "parallel_infer", "super_sampling"):
            if k in q:
                q[k] = str(q[k]).lower() in ("1", "true")
        if "timestamps" in q:
            q["timestamps"] = parse_timestamps(q["timestamps"])
        return await respond(q)

    async def tts_post(request):
        return await respond(await request.json())
    # this module's annotations are strings, and FastAPI cannot resolve one that names a local import (it then asks for a
    # query parameter "request" and answers 422): hand it the class itself
    for route, fn in ((app.get, tts_get), (app.post, tts_post)):
        fn.__annotations__["request"] = Request
        route("/tts")(fn)
    return app
