"""Mirror of the reference CLI `GPT_SoVITS/inference_cli.py` (flags :100-122, `synthesize` :11-24,
writes `<output_path>/output.wav` :95-96) on the HIP engines.

The reference CLI goes through `inference_webui.get_tts_wav`: a single-utterance loop that uses the
*naive* AR entry point (EOS masked for the first 11 steps, t2s_model.py:888-889), decodes each sentence
separately, peak-normalises, appends 0.3 s of zeros and scales by 32767 (inference_webui.py:977-1001).
`get_tts_wav` below restates that glue.

Front-end (`--frontend`, an addition to the reference's flags: the reference hard-wires its third-party G2P packages):
    symbols              the text files hold phoneme symbols separated by white space (gsv.text.g2p.SymbolG2P): runs the
                         whole pipeline with no G2P package at all
    cmudict:<file>       English by look-up in a CMUdict-format dictionary (gsv.text.g2p.DictG2P; the reference ships
                         text/cmudict.rep in that format)
    pkg.module:factory   factory() returns an object with text_to_segments(text, language) and, optionally,
                         reference(ref_audio_path, vits_model); it may also just call gsv.text.cleaner.register_g2p
The built-in front-end is `BuiltinFrontend`: gsv.TTS_infer_pack.TextPreprocessor for the text and, for the reference audio,
WAV -> 16 kHz -> HuBERT-base (gsv.feature_extractor.cnhubert, weights from --cnhubert_base_path) -> extract_latent, and
gsv.module.mel_processing.spectrogram_torch (reference inference_webui.py:590-640, 806-830).
"""
from __future__ import annotations

import argparse
import os
import wave
from typing import Iterator, Optional, Tuple

import numpy as np
import torch

from .AR.models.t2s_model import Text2SemanticDecoder
from .module.models import SynthesizerTrn
from .TTS_infer_pack.TTS import load_sovits_new


def get_tts_wav(t2s: Text2SemanticDecoder, vits: SynthesizerTrn, prompt_semantic: torch.Tensor, refer_spec,
                prompt_segment: dict, segments, top_k: int = 20, top_p: float = 1.0, temperature: float = 1.0,
                speed: float = 1.0, hz: int = 50, max_sec: int = 54, pause_second: float = 0.3,
                sampling_rate: int = 32000, seed: int = 0, loudness: Optional[float] = None, loudness_scope: str = "fragment",
                loudness_peak: float = 0.0, sample_rate: Optional[int] = None,
                timestamps: Optional[list] = None) -> Iterator[Tuple[int, np.ndarray]]:
    """reference inference_webui.py:751-1001 restated for pre-tokenised input; yields (32000, int16).
    loudness (LUFS) and sample_rate are additions: with `loudness` the float sentences and their pauses
    go through audio_io.postprocess_sentences instead of the host conversion -- metered and scaled on the device per fragment
    or per sentence, resampled to `sample_rate` when given, int16 as trunc(x * 32768) saturating -- and (rate, int16) is
    yielded.  timestamps (a list): the speech marks of the output, one record per sentence with its
    phonemes, are appended to it -- each decode then also aligns its phonemes; the audio does not depend on it."""
    dev = t2s.device
    sents = []
    zero = np.zeros(int(sampling_rate * pause_second), dtype=np.float32)
    audio = []
    for si, seg in enumerate(segments):
        phones = list(prompt_segment["phones"]) + list(seg["phones"])
        pb, sb = prompt_segment.get("bert_features"), seg.get("bert_features")
        bert = None
        if pb is not None or sb is not None:
            pb = torch.zeros(1024, len(prompt_segment["phones"])) if pb is None else pb
            sb = torch.zeros(1024, len(seg["phones"])) if sb is None else sb
            bert = torch.cat([pb, sb], 1).unsqueeze(0)
        ids = torch.LongTensor(phones).unsqueeze(0)
        pred, idx = t2s.infer_panel(ids, torch.LongTensor([ids.shape[-1]]), prompt_semantic.view(1, -1).to(dev), bert,
                                    top_k=top_k, top_p=top_p, temperature=temperature, early_stop_num=hz * max_sec,
                                    seed=seed + si)
        pred = pred[:, -idx:].unsqueeze(0) if idx > 0 else pred[:, :0].unsqueeze(0)
        if pred.shape[-1] == 0:
            continue
        wav = vits.decode(pred, torch.LongTensor(seg["phones"]).unsqueeze(0), refer_spec, speed=speed, seed=seed + si,
                          **({} if timestamps is None else {"align": True}))[0, 0].float().cpu().numpy()
        if timestamps is not None:
            ends, score = vits.last_alignment[0]
            sents.append(dict(index=si, text=seg.get("norm_text"), n_samples=int(wav.shape[0]), phones=list(seg["phones"]),
                              nf=2 * int(pred.shape[-1]), ends=ends, score=score,
                              **({"word2ph": seg["word2ph"]} if seg.get("word2ph") is not None else {})))
        peak = np.abs(wav).max()
        if peak > 1:
            wav = wav / peak
        audio.append(wav)
        audio.append(zero)
    if not audio:
        return
    if timestamps is not None:
        from .timestamps import build_marks
        timestamps += build_marks(sents, sampling_rate, zero.shape[0])
    if loudness is not None:
        from .audio_io import postprocess_sentences
        rate = sampling_rate if sample_rate is None else int(sample_rate)
        pcm, _ = postprocess_sentences(audio[0::2], zero.shape[0], sampling_rate, rate, None, dev, loudness, loudness_scope,
                                       loudness_peak)
        yield rate, pcm
        return
    yield sampling_rate, (np.concatenate(audio, 0) * 32767).astype(np.int16)


# reference inference_webui.py:140-160 (i18n keys are the Chinese labels themselves)
dict_language_v1 = {"中文": "all_zh", "英文": "en", "日文": "all_ja", "中英混合": "zh", "日英混合": "ja", "多语种混合": "auto"}
dict_language_v2 = dict(dict_language_v1, **{"粤语": "all_yue", "韩文": "all_ko", "粤英混合": "yue", "韩英混合": "ko",
                                               "多语种混合(粤语)": "auto_yue"})


class BuiltinFrontend:
    """text -> segments through TextPreprocessor with the registered G2P back-ends; reference audio -> (prompt_semantic,
    refer_spec) through the HIP HuBERT engine and spectrogram."""

    def __init__(self, device, cnhubert_base_path=None, hubert_state_dict=None, bert_fn=None, version="v2", cut="cut0"):
        from .TTS_infer_pack.TextPreprocessor import TextPreprocessor
        self.device, self.version, self.cut = torch.device(device), version, cut
        self.tp = TextPreprocessor(bert_fn=bert_fn, device="cpu")
        self._hubert = None
        self._hubert_src = (cnhubert_base_path, hubert_state_dict)

    def text_to_segments(self, text: str, language: str):
        lang = (dict_language_v1 if self.version == "v1" else dict_language_v2).get(language, language)
        return self.tp.preprocess(text, lang, self.cut, self.version)

    def reference(self, ref_audio_path: str, vits_model):
        from .audio_io import load_wav, resample
        from .feature_extractor.cnhubert import CNHubert
        from .module.mel_processing import spectrogram_torch
        if self._hubert is None:
            base, sd = self._hubert_src
            if base is None and sd is None:
                raise FileNotFoundError("--cnhubert_base_path (directory with the chinese-hubert-base weights) is required")
            self._hubert = CNHubert(base, device=self.device, state_dict=sd)
        raw, sr = load_wav(ref_audio_path)
        mono = raw.mean(0)
        wav16k = resample(mono, sr, 16000)
        if wav16k.shape[0] > 160000 or wav16k.shape[0] < 48000:
            raise OSError("参考音频在3~10秒范围外，请更换！")                 # inference_webui.py:812-814
        zero = np.zeros(int(32000 * 0.3), dtype=np.float32)
        w = torch.from_numpy(np.concatenate([wav16k, zero])).to(self.device)
        ssl = self._hubert.model(w.unsqueeze(0))["last_hidden_state"].transpose(1, 2)
        prompt_semantic = vits_model.extract_latent(ssl)[0, 0]
        audio = torch.from_numpy(resample(mono, sr, 32000)).unsqueeze(0).to(self.device)
        maxx = float(audio.abs().max())
        if maxx > 1:
            audio = audio / min(2.0, maxx)
        spec = spectrogram_torch(audio, 2048, 32000, 640, 2048, center=False)
        return prompt_semantic, spec


def make_frontend(spec: str, device, cnhubert_base_path=None, version="v2"):
    """--frontend value -> front-end object (see the module docstring)"""
    from .text import cleaner, g2p
    if spec == "symbols":
        for lang in ("zh", "ja", "en", "ko", "yue"):
            cleaner.register_g2p(lang, _SymbolAny(lang))
        return BuiltinFrontend(device, cnhubert_base_path, version=version)
    if spec.startswith("cmudict:"):
        cleaner.register_g2p("en", g2p.DictG2P(spec[len("cmudict:"):]))
        return BuiltinFrontend(device, cnhubert_base_path, version=version)
    if ":" in spec:
        import importlib
        mod, fn = spec.split(":", 1)
        obj = getattr(importlib.import_module(mod), fn)()
        if obj is None or not hasattr(obj, "text_to_segments"):
            return BuiltinFrontend(device, cnhubert_base_path, version=version)       # the factory only registered G2P back-ends
        if not hasattr(obj, "reference"):
            obj.reference = BuiltinFrontend(device, cnhubert_base_path, version=version).reference
        return obj
    raise ValueError(f"--frontend {spec!r}: expected 'symbols', 'cmudict:<file>' or 'pkg.module:factory'")


class _SymbolAny:
    """SymbolG2P for any language: zh / yue must also return word2ph (one entry per character of the normalised text)."""

    def __init__(self, lang):
        self.lang = lang

    def text_normalize(self, text):
        return " ".join(text.split())

    def g2p(self, norm):
        ph = norm.split()
        if self.lang not in ("zh", "yue"):
            return ph
        w2p = [0] * len(norm)
        pos = 0
        for tok in ph:                      # every symbol is charged to its first character
            pos = norm.index(tok, pos)
            w2p[pos] += 1
            pos += len(tok)
        return ph, w2p


def synthesize(GPT_model_path, SoVITS_model_path, ref_audio_path, ref_text_path, ref_language, target_text_path,
               target_language, output_path, bert_path=None, cnhubert_base_path=None, gpu_number="0", is_half=True,
               frontend=None, sample_rate=None, loudness=None, loudness_scope="fragment", loudness_peak=0.0,
               timestamps_path=None):
    if frontend is None:
        raise ValueError("pass `frontend` (an object, or a --frontend string for make_frontend): the reference's G2P "
                         "packages are third-party and not part of this build (see the module docstring)")
    device = f"cuda:{int(gpu_number)}"
    if isinstance(frontend, str):
        frontend = make_frontend(frontend, device, cnhubert_base_path)
    with open(ref_text_path, "r", encoding="utf-8") as f:
        ref_text = f.read()
    with open(target_text_path, "r", encoding="utf-8") as f:
        target_text = f.read()
    dtype = torch.float16 if is_half else torch.float32
    s1 = torch.load(GPT_model_path, map_location="cpu", weights_only=True)
    t2s = Text2SemanticDecoder(s1["config"], device=device, dtype=dtype, max_batch=1, max_seq=2048)
    t2s.load_state_dict(s1["weight"])
    s2 = load_sovits_new(SoVITS_model_path)
    hps = s2["config"]
    mcfg = dict(hps["model"])
    version = mcfg.pop("version", "v2")
    vits = SynthesizerTrn(hps["data"]["filter_length"] // 2 + 1, hps["train"]["segment_size"] // hps["data"]["hop_length"],
                          n_speakers=hps["data"]["n_speakers"], version=version if version in ("v1", "v2") else "v2",
                          device=device, dtype=dtype, **mcfg)
    vits.load_state_dict(s2["weight"])
    prompt_semantic, refer_spec = frontend.reference(ref_audio_path, vits)
    prompt_seg = frontend.text_to_segments(ref_text, ref_language)[0]
    segments = frontend.text_to_segments(target_text, target_language)
    marks = None if timestamps_path is None else []
    result = list(get_tts_wav(t2s, vits, prompt_semantic, refer_spec, prompt_seg, segments,
                              max_sec=s1["config"]["data"]["max_sec"], loudness=loudness, loudness_scope=loudness_scope,
                              loudness_peak=loudness_peak, sample_rate=sample_rate if loudness is not None else None,
                              **({} if marks is None else {"timestamps": marks})))
    if result:
        sr, audio = result[-1]
        if sample_rate is not None and int(sample_rate) != sr:       # --sample_rate: resampled on the device
            from .audio_io import convert_pcm                        # (with --loudness get_tts_wav has done both: sr is the rate)
            audio, sr = convert_pcm(audio, sr, int(sample_rate), device=device), int(sample_rate)
        os.makedirs(output_path, exist_ok=True)
        out = os.path.join(output_path, "output.wav")
        with wave.open(out, "wb") as w:            # 16-bit PCM, what soundfile.write produces for int16 (inference_cli.py:95-96)
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(sr)
            w.writeframes(audio.tobytes())
        print(f"Audio saved to {out}")
        if marks is not None:                      # --timestamps PATH: the speech marks of output.wav as JSON (seconds)
            import json
            from .timestamps import to_json
            with open(timestamps_path, "w", encoding="utf-8") as f:
                json.dump(to_json(marks), f, ensure_ascii=False)
            print(f"Timestamps saved to {timestamps_path}")


def main(argv=None):
    p = argparse.ArgumentParser(description="GPT-SoVITS Command Line Tool")
    p.add_argument("--gpt_model", required=True, help="Path to the GPT model file")
    p.add_argument("--sovits_model", required=True, help="Path to the SoVITS model file")
    p.add_argument("--ref_audio", required=True, help="Path to the reference audio file")
    p.add_argument("--ref_text", required=True, help="Path to the reference text file")
    p.add_argument("--ref_language", required=True, choices=["中文", "英文", "日文"], help="Language of the reference audio")   # as the reference (:107-108)
    p.add_argument("--target_text", required=True, help="Path to the target text file")
    p.add_argument("--target_language", required=True, choices=["中文", "英文", "日文", "中英混合", "日英混合", "多语种混合"],
                   help="Language of the target text")
    p.add_argument("--output_path", required=True, help="Path to the output directory")
    p.add_argument("--bert_path", default=None)
    p.add_argument("--cnhubert_base_path", default=None)
    p.add_argument("--gpu_number", default="0")
    p.add_argument("--is_half", default="True")
    p.add_argument("--frontend", default=os.environ.get("GSV_FRONTEND", "symbols"),
                   help="text front-end: 'symbols' (text files hold phoneme symbols), 'cmudict:<file>' (English dictionary G2P) "
                        "or 'pkg.module:factory' (default: $GSV_FRONTEND or 'symbols')")
    p.add_argument("--sample_rate", type=int, default=None,
                   help="sample rate of output.wav in Hz (an addition to the reference's flags; default: the model's, 32000)")
    p.add_argument("--loudness", type=float, default=None,
                   help="normalise output.wav to this programme loudness in LUFS (ITU-R BS.1770, -70 .. 0; default: off)")
    p.add_argument("--loudness_scope", default="fragment", choices=["fragment", "sentence"],
                   help="what is metered together and gets one gain: the whole output with its pauses, or each sentence")
    p.add_argument("--timestamps", default=None, metavar="PATH",
                   help="write the speech marks of output.wav (sentence and phoneme times in seconds, with a confidence) as JSON")
    p.add_argument("--loudness_peak", type=float, default=0.0, help="ceiling of the normalised peak in dBFS (<= 0, default 0)")
    a = p.parse_args(argv)
    if a.sample_rate is not None and a.sample_rate <= 0:
        p.error("--sample_rate must be positive")
    if a.loudness is not None and not -70.0 <= a.loudness <= 0.0:
        p.error("--loudness is a target in LUFS, -70 .. 0")
    if a.loudness_peak > 0.0:
        p.error("--loudness_peak is a ceiling in dBFS, at most 0")
    synthesize(a.gpt_model, a.sovits_model, a.ref_audio, a.ref_text, a.ref_language, a.target_text, a.target_language,
               a.output_path, a.bert_path, a.cnhubert_base_path, a.gpu_number, str(a.is_half).lower() in ("true", "1"),
               frontend=a.frontend, sample_rate=a.sample_rate, loudness=a.loudness, loudness_scope=a.loudness_scope,
               loudness_peak=a.loudness_peak, **({} if a.timestamps is None else {"timestamps_path": a.timestamps}))


if __name__ == "__main__":
    main()
