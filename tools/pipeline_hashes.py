"""Bit-equality anchor of the host pipeline across a commit: the small synthetic v2, v2Pro, v3 and v4 pipelines of the
run_batch GPU tests, in fp32 and fp16, run one fixed request list through TTS.run(), TTS.run_batch(),
run_batch(shared_sovits=True) and run_batch(shared_cfm=True), and every returned int16 array is printed as one sha256 line.
The list covers two voices, two to_batch batches, a prompt-free request (v2 / v2Pro), speed_factor 1.25,
parallel_infer=False, a guided and an unguided request (v3 / v4) and return_fragment=True through run().

    python tools/pipeline_hashes.py > after.txt        # once on each of the two commits; the files must be identical

Only the public request API is used, so the same file runs on either side of a refactor of gsv/TTS_infer_pack/TTS.py.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gpt-sovits_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def requests_for(version, half):
    """[(voice components, request)] and the index of the request that also goes through run(return_fragment=True)"""
    from test_run_batch_cfm_gpu import _voice
    from test_run_batch_gpu import _segs, _voice_args
    if version in ("v3", "v4"):
        va, vb = _voice(0, 8, 6, 14, version), _voice(1, 14, 4, 31, version)
        base = dict(top_k=5, sample_steps=2, fragment_interval=0.01)
        reqs = [(va, dict(base, segments=_segs(20, [9, 5]), batch_size=2, seed=3)),
                (vb, dict(base, segments=_segs(22, [11, 6, 8]), batch_size=2, seed=5, inference_cfg_rate=0.7)),
                (va, dict(base, segments=_segs(24, [10]), speed_factor=1.25, seed=7)),
                (vb, dict(base, segments=_segs(23, [8, 5]), batch_size=2, parallel_infer=False, seed=8))]
    else:
        va, vb = _voice_args(0, 8, 6, version), _voice_args(1, 23, 4, version)
        vfree = _voice_args(3, 5, 0, version, prompt_free=True)
        base = dict(top_k=5, top_p=1.0, temperature=1.0, repetition_penalty=1.35, fragment_interval=0.01)
        reqs = [(va, dict(base, segments=_segs(0, [9, 5]), seed=3)),
                (vb, dict(base, segments=_segs(2, [11, 6, 8]), batch_size=2, seed=5)),
                (vfree, dict(base, segments=_segs(3, [6, 9]), batch_size=2, seed=6)),
                (va, dict(base, segments=_segs(4, [10]), speed_factor=1.25, seed=7)),
                (vb, dict(base, segments=_segs(5, [8, 5]), batch_size=2, parallel_infer=False, seed=8))]
    if half:
        for kw in {id(kw): kw for kw, _ in reqs}.values():
            kw["refer_spec"] = [s.half() for s in kw["refer_spec"]]
    return reqs, 1


def build(version, half):
    if version in ("v3", "v4"):
        from test_pipeline_v3_gpu import _build
        return _build(version, half)[0]
    from test_run_batch_gpu import _build
    tts = _build(version)
    if half:
        tts.enable_half_precision(True, save=False)
    return tts


def main():
    import torch
    assert torch.cuda.is_available(), "pipeline_hashes.py runs the HIP engines: it needs the GPU"
    for version in ("v2", "v2Pro", "v3", "v4"):
        for half in (False, True):
            tts = build(version, half)
            reqs, frag = requests_for(version, half)
            tag = f"{version} {'fp16' if half else 'fp32'}"

            def show(mode, r, k, sr, audio):
                assert audio.dtype == np.int16
                print(f"{tag} {mode} request {r} array {k}: sr {sr} samples {audio.size} "
                      f"sha256 {hashlib.sha256(np.ascontiguousarray(audio).tobytes()).hexdigest()}", flush=True)

            for r, (kw, req) in enumerate(reqs):
                tts.set_prompt_cache(**kw)
                for k, (sr, audio) in enumerate(tts.run(dict(req))):
                    show("run", r, k, sr, audio)
            kw, req = reqs[frag]
            tts.set_prompt_cache(**kw)
            for k, (sr, audio) in enumerate(tts.run(dict(req, return_fragment=True))):
                show("run-fragments", frag, k, sr, audio)
            voices = {id(kw): tts.make_voice(**kw) for kw, _ in reqs}
            batch = [dict(req, voice=voices[id(kw)]) for kw, req in reqs]
            for mode, flags in (("run_batch", {}), ("run_batch-shared_sovits", {"shared_sovits": True}),
                                ("run_batch-shared_cfm", {"shared_cfm": True})):
                for r, (sr, audio) in enumerate(tts.run_batch([dict(b) for b in batch], **flags)):
                    show(mode, r, 0, sr, audio)
            del tts
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
