"""Host-side mirror of the reference pipeline API `TTS_infer_pack.TTS` (reference
GPT_SoVITS/TTS_infer_pack/TTS.py: `TTS_Config`:217, `TTS`:412, `run`:984, `to_batch`:842,
`recovery_order`:957, `audio_postprocess`:1377, `using_vocoder_synthesis`:1431, `..._batched_infer`:1496,
`sola_algorithm`:1611), v1/v2 and v3/v4 paths, on the HIP engines.

What is kept: the `run(inputs) -> generator of (sr, int16 ndarray)` contract with the reference's
keys and defaults, length-bucketed batching, AR -> one time-axis-concatenated `decode` per batch,
per-fragment peak normalisation, fragment silence, original-order recovery, x32768 int16 scaling,
the error protocol (1 s of silence then re-raise) and `stop()`.

Front-ends are separate modules this class wires together: `set_ref_audio(path)` =
WAV -> HuBERT engine -> `extract_latent` (prompt tokens), `spectrogram_torch` (reference spectrogram), for v2Pro the ERes2NetV2
speaker embedding, for v3 / v4 the reference mel; `run({"text": ...})` goes through `TextPreprocessor` (pluggable G2P and
language splitter, BERT engine for zh).  Pre-tokenised `segments` and `set_prompt_cache(...)` remain as the model-level entry.
"""
from __future__ import annotations

import collections
import contextlib
import math
import numbers
import os
import random
import time
import traceback
from typing import Callable, Dict, Generator, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F

from ..AR.models.t2s_model import Text2SemanticDecoder
from .._lib import CFM_SESSION_MAX_ROWS
from ..module.models import CFM, SynthesizerTrn, SynthesizerTrnV3, cfg_guided
from ..process_ckpt import load_sovits_new  # noqa: F401  (reference process_ckpt.py:129-138; re-exported)
from ..timestamps import build_marks


spec_min, spec_max = -12, 2          # reference TTS.py:55-56


def norm_spec(x):
    return (x - spec_min) / (spec_max - spec_min) * 2 - 1


def denorm_spec(x):
    return (x + 1) / 2 * (spec_max - spec_min) + spec_min


def mel_fn(x):
    """reference TTS.py:67-79 (v3: 24 kHz, n_fft 1024, hop 256, 100 mels)"""
    from ..module.mel_processing import mel_spectrogram_torch
    return mel_spectrogram_torch(x, n_fft=1024, win_size=1024, hop_size=256, num_mels=100, sampling_rate=24000, fmin=0, fmax=None,
                                 center=False)


def mel_fn_v4(x):
    """reference TTS.py:81-93 (v4: 32 kHz, n_fft 1280, hop 320, 100 mels)"""
    from ..module.mel_processing import mel_spectrogram_torch
    return mel_spectrogram_torch(x, n_fft=1280, win_size=1280, hop_size=320, num_mels=100, sampling_rate=32000, fmin=0, fmax=None,
                                 center=False)


class NO_PROMPT_ERROR(Exception):
    pass


def set_seed(seed: int) -> int:
    """reference TTS.py:180-205: -1 -> random seed; seeds python/numpy/torch."""
    seed = int(seed)
    seed = seed if seed != -1 else random.randint(0, 2 ** 32 - 1)
    os.environ["PYTHONHASHSEED"] = str(seed)
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    return seed


def silence() -> Tuple[int, np.ndarray]:
    """what run() / run_batch return for no text, a stop and an error (reference TTS.py:1132, 1334, 1340, 1355): 1 s at 16 kHz"""
    return 16000, np.zeros(16000, dtype=np.int16)


def early_stop_num(configs) -> float:
    """the AR decode horizon in tokens (reference TTS.py:1224): hz * max_sec of the AR checkpoint, 54 s where it names none"""
    return configs.hz * (configs.max_sec if configs.max_sec is not None else 54)


BEST_OF_MAX = 16            # candidates per sentence: row + 1024 * 15 fits the 24 bits the counter RNG's hash gives the row
BEST_OF_ROW_STRIDE = 1024   # candidate c of the sentence with the key (seed, row) draws with (seed, row + 1024 c)


def _mean_logprob(cand: dict) -> float:
    """mean log-probability of a candidate's `n` generated tokens, in float64 on the host; the finishing step's entry is not
    counted, and a candidate that generated nothing scores -inf"""
    n = int(cand["n"])
    if n <= 0:
        return float("-inf")
    lp = cand["logprobs"]
    lp = lp.detach().cpu().numpy() if torch.is_tensor(lp) else np.asarray(lp)
    return float(lp[:n].astype(np.float64).mean())


def select_candidate(cands: Sequence[dict]) -> int:
    """The default choice among the candidates of one sentence ("best_of").  Each is dict(tokens, logprobs, n, cut): the
    generated tokens, the log-probabilities of the taken tokens (n generated ones, then the finishing step), their count and
    whether the row was ended by early_stop_num, max_steps or the K/V arena instead of EOS.  Candidates that were not cut come
    before cut ones; among those the highest mean log-probability of the n generated tokens wins; ties go to the lowest index."""
    best, best_key = 0, None
    for i, c in enumerate(cands):
        key = (not c["cut"], _mean_logprob(c))
        if best_key is None or key > best_key:
            best, best_key = i, key
    return best


def check_best_of(o: dict, no_prompt: Optional[bool] = None) -> None:
    """ValueError unless the options' "best_of" (present only when the request named one other than 1) is an int in
    2 .. BEST_OF_MAX on a parallel decode with a prompt (no_prompt=None: the prompt is not known yet and not checked)"""
    if "best_of" not in o:
        return
    n = o["best_of"]
    if type(n) is not int or not 1 <= n <= BEST_OF_MAX:
        raise ValueError(f"best_of must be an int in 1..{BEST_OF_MAX}, got {n!r}")
    if "best_of_score" in o and not callable(o["best_of_score"]):
        raise ValueError("best_of_score must be a callable: candidates -> index")
    if not o["parallel_infer"]:
        raise ValueError("best_of > 1 needs parallel_infer=True: the naive loop decodes a sentence alone")
    if no_prompt:
        raise ValueError("best_of > 1 needs a prompt: the prompt-free loop decodes a sentence alone")


def choose_candidate(o: dict, cands: Sequence[dict]) -> Tuple[int, List[dict]]:
    """(index of the chosen candidate, the record of the choice: dict(n, mean_logprob, cut, chosen) per candidate) under the
    request's "best_of_score" callable, or select_candidate without one"""
    k = o.get("best_of_score", select_candidate)(cands)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k < len(cands):
        raise ValueError(f"best_of_score returned {k!r} for {len(cands)} candidates")
    return int(k), [dict(n=int(c["n"]), mean_logprob=_mean_logprob(c), cut=bool(c["cut"]), chosen=i == k)
                    for i, c in enumerate(cands)]


def plan_cfm_session(rows: Sequence[Tuple[int, bool]], cap: int) -> List[Tuple[List[int], int]]:
    """The schedule of a flow-matching session (CFM.open_session) for `rows` = [(sample_steps, guided)] in arrival order and
    a cap of `cap` live DiT rows, a guided row counting 2 (itself and its unconditioned twin).  Pure: no engine, no tensors.
    Returns [(admit, k)]: before the call step(k) the rows `admit` (indices into `rows`, possibly none) are admitted.
    Admission is FIFO -- a row never overtakes an earlier one, so a guided row at the head of the queue waits for two free
    DiT rows even when a later unguided row would fit the one that is free -- and as many rows as fit are admitted at once.
    Every step() call runs until the next live row finishes (k = the smallest number of steps any live row still has to
    take), so a place is refilled as soon as it is free.  Every row takes exactly its sample_steps steps."""
    cap = int(cap)
    need = [2 if g else 1 for _, g in rows]
    for i, (steps, _) in enumerate(rows):
        if int(steps) < 1:
            raise ValueError(f"row {i}: sample_steps {steps} < 1")
        if need[i] > cap:
            raise ValueError(f"row {i} needs {need[i]} DiT rows, the session has {cap}")
    schedule: List[Tuple[List[int], int]] = []
    left: Dict[int, int] = {}           # live row -> steps it still has to take
    nxt, used = 0, 0
    while nxt < len(rows) or left:
        admit = []
        while nxt < len(rows) and used + need[nxt] <= cap:
            admit.append(nxt)
            left[nxt] = int(rows[nxt][0])
            used += need[nxt]
            nxt += 1
        k = min(left.values())
        schedule.append((admit, k))
        for i in list(left):
            left[i] -= k
            if left[i] == 0:
                del left[i]
                used -= need[i]
    return schedule


class TTS_Config:
    """The reference's TTS_Config surface (TTS.py:217-410): `configs` is a dict (the sections "v1" ... "v2ProPlus" and / or
    "custom", or directly the custom section's keys), a YAML file path, or None (defaults).  Differences, all forced by the
    platform: the default device is the GPU ("cuda:0", half precision on) instead of "cpu" -- there is no CPU path -- and a
    weights path that does not exist is kept as given (the engines take in-memory checkpoints too, `TTS.init_*_weights(state=)`)
    instead of silently falling back to the pretrained-model default.  `max_batch` / `max_seq` size the AR engine's K/V arena."""
    default_configs = {
        v: {"device": "cuda:0", "is_half": True, "version": v, "t2s_weights_path": "GPT_SoVITS/pretrained_models/" + t,
            "vits_weights_path": "GPT_SoVITS/pretrained_models/" + s_,
            "cnhuhbert_base_path": "GPT_SoVITS/pretrained_models/chinese-hubert-base",
            "bert_base_path": "GPT_SoVITS/pretrained_models/chinese-roberta-wwm-ext-large"}
        for v, t, s_ in (("v1", "s1bert25hz-2kh-longer-epoch=68e-step=50232.ckpt", "s2G488k.pth"),
                         ("v2", "gsv-v2final-pretrained/s1bert25hz-5kh-longer-epoch=12-step=369668.ckpt", "gsv-v2final-pretrained/s2G2333k.pth"),
                         ("v3", "s1v3.ckpt", "s2Gv3.pth"), ("v4", "s1v3.ckpt", "gsv-v4-pretrained/s2Gv4.pth"),
                         ("v2Pro", "s1v3.ckpt", "v2Pro/s2Gv2Pro.pth"), ("v2ProPlus", "s1v3.ckpt", "v2Pro/s2Gv2ProPlus.pth"))
    }
    v1_languages = ["auto", "en", "zh", "ja", "all_zh", "all_ja"]
    v2_languages = ["auto", "auto_yue", "en", "zh", "ja", "yue", "ko", "all_zh", "all_ja", "all_yue", "all_ko"]
    _KEYS = ("device", "is_half", "version", "t2s_weights_path", "vits_weights_path", "bert_base_path", "cnhuhbert_base_path")

    def __init__(self, configs=None):
        from copy import deepcopy
        self.configs_path = os.path.join("GPT_SoVITS", "configs", "tts_infer.yaml")
        if configs in ["", None]:
            configs = {}
        if isinstance(configs, str):
            self.configs_path = configs
            configs = self._load_configs(configs)
        if not isinstance(configs, dict):
            raise TypeError("configs must be a dict, a YAML path or None")
        sections = deepcopy(self.default_configs)
        if any(k in configs for k in list(self.default_configs) + ["custom"]):
            sections.update(deepcopy(configs))
            custom = sections.get("custom", sections["v2"])
        else:                                   # the custom section's keys given directly
            if configs.get("version", "v2") not in sections:
                raise NotImplementedError(f"version {configs.get('version')} is not one of v1, v2, v2Pro, v2ProPlus, v3, v4")
            custom = dict(sections[configs.get("version", "v2")], **configs)
        self.default_configs = sections
        self.configs = dict(custom)
        self.device = torch.device(custom.get("device", "cuda:0"))
        self.is_half = bool(custom.get("is_half", True))
        self.version = custom.get("version", "v2")
        if self.version not in ("v1", "v2", "v2Pro", "v2ProPlus", "v3", "v4"):
            raise NotImplementedError(f"version {self.version} is not one of v1, v2, v2Pro, v2ProPlus, v3, v4")
        self.t2s_weights_path = custom.get("t2s_weights_path")
        self.vits_weights_path = custom.get("vits_weights_path")
        self.bert_base_path = custom.get("bert_base_path")
        self.cnhuhbert_base_path = custom.get("cnhuhbert_base_path")
        self.max_batch = int(custom.get("max_batch", 32))
        # K/V arena positions per row: the reference's 1500-step loop (t2s_model.py:694) + a 10 s prompt (250 tokens)
        # + phonemes of prompt and text; 2560 x 32 rows x 24 layers is 4 GB of fp16 K/V
        self.max_seq = int(custom.get("max_seq", 2560))
        self.use_vocoder = self.version in ("v3", "v4")     # TTS.py:519-521
        self.languages = self.v1_languages if self.version == "v1" else self.v2_languages
        self.max_sec = None
        self.hz: int = 50
        self.semantic_frame_rate: str = "25hz"
        self.segment_size: int = 20480
        self.filter_length: int = 2048
        self.sampling_rate: int = 32000
        self.hop_length: int = 640
        self.win_length: int = 2048
        self.n_speakers: int = 300
        self.update_configs()

    def _load_configs(self, configs_path: str) -> dict:
        import yaml
        if not os.path.exists(configs_path):
            self.configs = None
            self.save_configs(configs_path)          # reference :361-366: a missing file is created from the defaults
        with open(configs_path, "r", encoding="utf-8") as f:
            return yaml.load(f, Loader=yaml.SafeLoader) or {}

    def save_configs(self, configs_path: Optional[str] = None) -> None:
        import yaml
        from copy import deepcopy
        configs = deepcopy(self.default_configs)
        if getattr(self, "configs", None) is not None:
            configs["custom"] = self.update_configs()
        configs_path = configs_path or self.configs_path
        d = os.path.dirname(configs_path)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(configs_path, "w") as f:
            yaml.dump(configs, f)

    def update_configs(self) -> dict:
        self.config = {"device": str(self.device), "is_half": self.is_half, "version": self.version,
                       "t2s_weights_path": self.t2s_weights_path, "vits_weights_path": self.vits_weights_path,
                       "bert_base_path": self.bert_base_path, "cnhuhbert_base_path": self.cnhuhbert_base_path}
        return self.config

    def update_version(self, version: str) -> None:
        self.version = version
        self.use_vocoder = version in ("v3", "v4")
        self.languages = self.v1_languages if self.version == "v1" else self.v2_languages

    def __str__(self):
        self.configs = self.update_configs()
        string = "TTS Config".center(100, "-") + "\n"
        for k, v in self.configs.items():
            string += f"{str(k).ljust(20)}: {str(v)}\n"
        return string + "-" * 100 + "\n"

    __repr__ = __str__

    def __hash__(self):
        return hash(self.configs_path)

    def __eq__(self, other):
        return isinstance(other, TTS_Config) and self.configs_path == other.configs_path

    @property
    def precision(self):
        return torch.float16 if self.is_half else torch.float32


class TTS:
    def __init__(self, configs=None):
        self.configs = configs if isinstance(configs, TTS_Config) else TTS_Config(configs)
        self.t2s_model: Optional[Text2SemanticDecoder] = None
        self.vits_model: Optional[SynthesizerTrn] = None
        self.text_frontend: Optional[Callable] = None
        # True: a request's raw text goes through TextPreprocessor.preprocess_many, so all its sentences' zh BERT features come
        # from one packed pass (BertFeature.batch) instead of one engine call per sentence
        self.batched_bert = False
        self.prompt_cache: dict = {
            "ref_audio_path": None, "prompt_semantic": None, "refer_spec": [], "prompt_text": None,
            "prompt_lang": None, "phones": None, "bert_features": None, "norm_text": None, "aux_ref_audio_paths": [],
        }
        self.stop_flag = False
        self.precision = self.configs.precision
        self._t2s_state = None
        self._vits_state = None
        self.vocoder = None
        self.sr_model = None                 # AP_BWE super-sampling (reference TTS.py:662-670), loaded on first use
        self.sr_model_not_exist = False
        self._sr_source = None
        self.cnhuhbert_model = None
        self.sv_model = None
        self.bert_model = None
        from .TextPreprocessor import TextPreprocessor
        self.text_preprocessor = TextPreprocessor(bert_fn=None, device="cpu")      # reference TTS.py:431-433
        self.vocoder_configs: dict = {"sr": None, "T_ref": None, "T_chunk": None, "upsample_rate": None, "overlapped_len": None}
        self._lora_voices: Dict[str, dict] = {}      # add_lora_voice: name -> {"slot", "engine", "state"}
        # "loudness": [{"lufs", "gain_db", "gain", "limited"} per span] per fragment delivered with it by the last run() /
        # run_batch(), or by the last audio_postprocess / postprocess_fragments call made directly (a server: its last call)
        self.last_loudness: list = []
        # speech marks of the last call (replaced, never extended): after run() the marks of the request, one record per sentence
        # ([] without "timestamps"; with return_fragment the last fragment's); after run_batch() one such list per request
        self.last_timestamps: list = []
        self.last_candidates: list = []              # "best_of": the choices of the last run / run_batch call, [request][batch][sentence]

    # ---- weights (reference TTS.py:484-603) ------------------------------------------------
    def init_t2s_weights(self, weights_path: Optional[str] = None, state: Optional[dict] = None):
        """`state` = {"weight": state_dict, "config": {...}} as stored in the reference's .ckpt
        (TTS.py:590-594); `weights_path` loads such a file with a non-executing loader."""
        if state is None:
            state = torch.load(weights_path, map_location="cpu", weights_only=True)
        self._t2s_state = state
        config = state["config"]
        self.configs.max_sec = config["data"]["max_sec"]
        self.configs.t2s_weights_path = weights_path
        m = Text2SemanticDecoder(config, device=self.configs.device, dtype=self.precision,
                                 max_batch=self.configs.max_batch, max_seq=self.configs.max_seq)
        m.load_state_dict(state["weight"])
        self.t2s_model = m

    def init_vits_weights(self, weights_path: Optional[str] = None, state: Optional[dict] = None, base_state: Optional[dict] = None):
        """reference TTS.py:484-582.  A v3 / v4 LoRA checkpoint (version code 03 / 04, or a `state` carrying "lora_rank") is merged
        into the base model's weights first (`process_ckpt.merge_lora_v3`); the base comes from `base_state` or from the
        configured pretrained path of that version, and a missing base raises FileExistsError like the reference (:491-493)."""
        from ..process_ckpt import get_sovits_version_from_path_fast, merge_lora_v3
        if state is None:
            state = load_sovits_new(weights_path)
        if_lora = "lora_rank" in state
        if weights_path is not None and not if_lora:
            if_lora = bool(get_sovits_version_from_path_fast(weights_path)[2])
        if if_lora:
            if base_state is None:
                path_sovits = self.configs.default_configs[self.configs.version]["vits_weights_path"]
                if not os.path.exists(path_sovits):
                    raise FileExistsError(f"{path_sovits}: SoVITS {self.configs.version} base model missing, cannot load the LoRA weights")
                base_state = load_sovits_new(path_sovits)
            state = dict(state, weight=merge_lora_v3(base_state["weight"], state["weight"], int(state["lora_rank"])))
        self._vits_state = state
        hps = state["config"]
        d = hps["data"]
        self.configs.filter_length = d["filter_length"]
        self.configs.segment_size = hps["train"]["segment_size"]
        self.configs.sampling_rate = d["sampling_rate"]
        self.configs.hop_length = d["hop_length"]
        self.configs.win_length = d["win_length"]
        self.configs.n_speakers = d["n_speakers"]
        self.configs.vits_weights_path = weights_path
        self.vits_model = self._build_vits_model(hps, state["weight"])
        v = self.vits_model
        self._lora_voices = {}           # they lived in the engines this call replaced: add_lora_voice again
        if getattr(v, "is_v2pro", False) and self.sv_model is None:
            from .. import sv
            if os.path.exists(sv.sv_path):            # reference TTS.py:487-488 loads it here; without the file: init_sv_model(state_dict=)
                self.init_sv_model()

    def _build_vits_model(self, hps: dict, weight: dict, cfm: Optional[CFM] = None) -> SynthesizerTrn:
        """the SoVITS engine of `hps` (a checkpoint's config) loaded with `weight`; `cfm` (v3 / v4): share that flow-matching
        decoder instead of building and loading a DiT (the encoder-side engine of a LoRA voice)"""
        d, mcfg = hps["data"], dict(hps["model"])
        mcfg.pop("version", None)
        extra = {}
        cls = SynthesizerTrn
        if self.configs.use_vocoder:
            cls = SynthesizerTrnV3
            if "dit" in hps:             # synthetic / test checkpoints may carry a smaller DiT than models.py:1219-1222
                extra["dit_kwargs"] = hps["dit"]
            if cfm is not None:
                extra["cfm"] = cfm
        v = cls(d["filter_length"] // 2 + 1, hps["train"]["segment_size"] // d["hop_length"],
                n_speakers=d["n_speakers"], version=self.configs.version, device=self.configs.device,
                dtype=self.precision, n_symbols=hps.get("n_symbols"), **extra, **mcfg)
        v.load_state_dict(weight)
        return v

    # ---- LoRA voices served beside the base model (v3 / v4) ---------------------------------------------------------
    def add_lora_voice(self, name: str, weights_path: Optional[str] = None, state: Optional[dict] = None) -> None:
        """A fine-tuned v3 / v4 voice (a LoRA checkpoint: version code 03 / 04, or `state` = {"weight", "lora_rank"[,
        "lora_alpha"]}) under `name`, next to the loaded base model instead of merged into it (init_vits_weights): requests
        select it with the key "lora_voice", and requests of different LoRA voices and of none share flow-matching passes.
        The adapters go into the base model's DiT engine (CFM.add_adapter).  Whatever else the file holds of the base
        model's parameters (the voice's own ref_enc / bridge / wns1 / ...) gets an encoder-side engine of its own, the base
        weights with these laid over them, around the same DiT; a file of adapters alone reuses the base one.  The DiT's
        own non-adapter weights stay the base model's: a file that changes them raises ValueError (merge it instead).
        init_vits_weights drops all LoRA voices; enable_half_precision / set_device add them again."""
        from ..process_ckpt import split_lora_v3
        if self.vits_model is None or not self.configs.use_vocoder:
            raise ValueError("add_lora_voice needs a loaded v3 / v4 base model (init_vits_weights)")
        if name is None or name in self._lora_voices:
            raise ValueError(f"LoRA voice {name!r}: " + ("a name is required" if name is None else "already added"))
        if state is None:
            state = load_sovits_new(weights_path)
        if "lora_rank" not in state:
            raise ValueError("not a LoRA checkpoint: no lora_rank")
        rank, alpha = int(state["lora_rank"]), state.get("lora_alpha")
        adapter, overrides = split_lora_v3(state["weight"], rank, alpha)
        base = self._vits_state["weight"]
        enc = {}
        for k, v in overrides.items():
            if k not in base:
                continue
            if not k.startswith("cfm."):
                enc[k] = v
            elif v.shape != base[k].shape or not torch.equal(v.to(base[k].dtype), base[k]):
                raise ValueError(f"LoRA voice {name!r} changes {k}, a DiT weight outside the adapters: merge it with "
                                 "init_vits_weights instead")
        cfm = self.vits_model.cfm
        slot = cfm.add_adapter(adapter, rank, alpha)
        engine = None
        if enc:
            try:
                weight = {k: v for k, v in base.items() if not k.startswith("cfm.")}
                weight.update(enc)
                engine = self._build_vits_model(self._vits_state["config"], weight, cfm=cfm)
            except Exception:
                cfm.remove_adapter(slot)
                raise
        self._lora_voices[name] = dict(slot=slot, engine=engine, state=state)

    def remove_lora_voice(self, name: str) -> None:
        if name not in self._lora_voices:
            raise ValueError(f"unknown LoRA voice {name!r}")
        v = self._lora_voices.pop(name)
        self.vits_model.cfm.remove_adapter(v["slot"])

    def _lora_voice(self, name: Optional[str]) -> Tuple[SynthesizerTrn, Optional[int]]:
        """a request's "lora_voice" -> (the engine of its decode_encp and style vector, its adapter slot); None: the base"""
        if name is None:
            return self.vits_model, None
        v = getattr(self, "_lora_voices", {}).get(name)
        if v is None:
            raise ValueError(f"unknown LoRA voice {name!r}: add_lora_voice first")
        return v["engine"] or self.vits_model, v["slot"]

    def init_vocoder(self, version: Optional[str] = None, state: Optional[dict] = None, weights_path: Optional[str] = None):
        """reference TTS.py:605-660: v3 -> BigVGAN-v2 24 kHz x256, v4 -> the HiFi-GAN `Generator` 48 kHz x480.
        `state` = {"config": vocoder hyper-parameters, "weight": state dict} (or a file holding the state dict)."""
        version = version or self.configs.version
        if state is None:
            state = {"weight": torch.load(weights_path, map_location="cpu", weights_only=True), "config": None}
        cfg = state.get("config")
        if version == "v3":
            from ..BigVGAN.bigvgan import BigVGAN
            from .. import synthetic as S
            h = dict(cfg or S.BIGVGAN_V2_24K_CONFIG)
            self.vocoder = BigVGAN(h, device=self.configs.device, dtype=self.precision)
            self.vocoder.load_state_dict(state["weight"])
            self.vocoder_configs.update(sr=24000, T_ref=468, T_chunk=934, upsample_rate=256, overlapped_len=12)
        elif version == "v4":
            from ..module.models import Generator as HifiGenerator
            from .. import synthetic as S
            h = dict(cfg or S.HIFIGAN_V4_CONFIG)
            self.vocoder = HifiGenerator(initial_channel=100, resblock="1", resblock_kernel_sizes=h["resblock_kernel_sizes"],
                                         resblock_dilation_sizes=h["resblock_dilation_sizes"], upsample_rates=h["upsample_rates"],
                                         upsample_initial_channel=h["upsample_initial_channel"],
                                         upsample_kernel_sizes=h["upsample_kernel_sizes"], gin_channels=0, is_bias=True,
                                         device=self.configs.device, dtype=self.precision)
            self.vocoder.load_state_dict(state["weight"])
            self.vocoder_configs.update(sr=48000, T_ref=500, T_chunk=1000, upsample_rate=480, overlapped_len=12)
        else:
            raise ValueError(f"no vocoder for version {version}")
        up = math.prod(h["upsample_rates"])
        if up != self.vocoder_configs["upsample_rate"]:      # reduced test vocoders
            self.vocoder_configs["upsample_rate"] = up
        for k in ("T_ref", "T_chunk", "overlapped_len", "sr"):
            if cfg and k in cfg:
                self.vocoder_configs[k] = cfg[k]

    def init_sr_model(self, checkpoint_file: Optional[str] = None, state: Optional[dict] = None, config: Optional[dict] = None):
        """reference TTS.py:662-670: the AP_BWE 24k -> 48k super-sampling model behind `super_sampling` (v3).  Loads once;
        `checkpoint_file` defaults to the reference's tools/AP_BWE_main/24kto48k/g_24kto48k.zip (relative to the working
        directory, with config.json beside it); `state` = {"generator": state_dict} plus `config` replace the file for tests.
        The engine dtype follows configs.is_half like every other engine here (the reference keeps this model in fp32).
        A missing checkpoint raises FileNotFoundError naming the path (the reference prints a message and fails later)."""
        if self.sr_model is not None and checkpoint_file is None and state is None:
            return
        from ..tools.audio_sr import AP_BWE, DEFAULT_CHECKPOINT
        if state is None and checkpoint_file is None and self._sr_source is not None:
            checkpoint_file, state, config = self._sr_source
        if state is None:
            checkpoint_file = checkpoint_file or DEFAULT_CHECKPOINT
        self.sr_model = AP_BWE(self.configs.device, checkpoint_file=checkpoint_file, state=state, config=config, dtype=self.precision)
        self._sr_source = (checkpoint_file, state, config)
        self.sr_model_not_exist = False

    # ---- prompt cache (replaces set_ref_audio's HuBERT/STFT front-end, TTS.py:737-819) ---------
    def set_prompt_cache(self, prompt_semantic: torch.Tensor, refer_spec: Sequence[torch.Tensor],
                         phones: Optional[List[int]] = None, bert_features: Optional[torch.Tensor] = None,
                         norm_text: str = "", ref_mel: Optional[torch.Tensor] = None,
                         sv_emb: Optional[Sequence[torch.Tensor]] = None):
        """`ref_mel` (v3/v4 only): the log-mel of the reference audio as `mel_fn` / `mel_fn_v4` return it ([1, 100, Tm],
        TTS.py:67-88, 1453); `set_ref_audio` computes it from the waveform (`mel_fn` / `mel_fn_v4`), this is the model-level entry."""
        self.prompt_cache["ref_mel"] = ref_mel
        # v2Pro / v2ProPlus: one speaker-verification embedding [1, 20480] per reference spectrogram (reference sv.py:11-32,
        # TTS.py:790-800 keeps it beside the spectrogram); `set_ref_audio` computes it with gsv.sv.SV (ERes2NetV2)
        self.prompt_cache["sv_emb"] = list(sv_emb) if sv_emb is not None else None
        self.prompt_cache["prompt_semantic"] = prompt_semantic.to(self.configs.device) if prompt_semantic is not None else None
        # the spectrograms go to the device ONCE here (the engine caches the style vector per reference and keys the
        # cache on these tensors), and a new prompt always drops the engine's cached reference terms
        self.prompt_cache["refer_spec"] = [(s.to(self.configs.device), None) for s in refer_spec]
        if self.vits_model is not None:
            self.vits_model.invalidate_refer()
        self.prompt_cache["phones"] = phones
        self.prompt_cache["bert_features"] = bert_features
        self.prompt_cache["norm_text"] = norm_text

    # ---- device / precision (reference TTS.py:677-735) -----------------------------------------------------------
    def enable_half_precision(self, enable: bool = True, save: bool = True):
        """reference TTS.py:677-713: switch every model between fp16 and fp32.  The HIP engines hold their weights in the
        compute dtype, so the models are rebuilt from the retained checkpoints."""
        if str(self.configs.device) == "cpu" and enable:
            raise RuntimeError("half precision needs the GPU")
        if bool(enable) == self.configs.is_half:
            return
        self.configs.is_half = bool(enable)
        self.precision = self.configs.precision
        if save:
            self.configs.save_configs()
        self._rebuild_models()

    def set_device(self, device, save: bool = True):
        """reference TTS.py:715-735: move every model to `device` (another MI355X: there is no CPU path)."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("gsv engines run on an MI355X (cuda/HIP device) only; there is no CPU path")
        self.configs.device = device
        if save:
            self.configs.save_configs()
        self._rebuild_models()

    def _rebuild_models(self):
        if self._t2s_state is not None:
            self.t2s_model = None
            self.init_t2s_weights(self.configs.t2s_weights_path, state=self._t2s_state)
        if self._vits_state is not None:
            self.vits_model = None
            lora_voices = self._lora_voices
            self.init_vits_weights(self.configs.vits_weights_path, state=self._vits_state)
            for name, v in lora_voices.items():
                self.add_lora_voice(name, state=v["state"])
        if getattr(self, "_hubert_state", None) is not None:
            self.init_cnhuhbert_weights(state_dict=self._hubert_state)
        if self.sr_model is not None:               # reference TTS.py:734-735 moves it; here it follows the dtype as well
            self.sr_model.to(self.configs.device, self.precision)
        if getattr(self, "_bert_state", None) is not None:
            self.init_bert_weights(state_dict=self._bert_state[0], vocab=self._bert_state[1])
        for k in ("prompt_semantic",):
            if self.prompt_cache.get(k) is not None:
                self.prompt_cache[k] = self.prompt_cache[k].to(self.configs.device)
        self.prompt_cache["refer_spec"] = [(sp.to(self.configs.device), a) for sp, a in self.prompt_cache["refer_spec"]]

    def init_bert_weights(self, base_path: Optional[str] = None, state_dict: Optional[dict] = None, vocab=None):
        """chinese-roberta-wwm-ext-large for zh text (reference TTS.py:472-482, TextPreprocessor.py:191-204): hidden_states[-3]
        per character.  `state_dict` / `vocab` (list of tokens) replace the directory for tests."""
        from ..feature_extractor.bert import BertFeature
        self.bert_model = BertFeature(base_path, device=self.configs.device, state_dict=state_dict, vocab=vocab)
        self._bert_state = (state_dict, vocab) if state_dict is not None else None
        self.text_preprocessor.bert_fn = self.bert_model
        self.configs.bert_base_path = base_path

    # ---- reference-audio front-end (reference TTS.py:462-482, 737-819) -------------------------------------------
    def init_cnhuhbert_weights(self, base_path: Optional[str] = None, state_dict: Optional[dict] = None):
        """HuBERT-base content encoder (reference TTS.py:462-470; feature_extractor/cnhubert.py).  `state_dict` = a
        transformers.HubertModel state dict (tests, synthetic weights); `base_path` = directory with pytorch_model.bin /
        model.safetensors."""
        from ..feature_extractor.cnhubert import CNHubert
        self.cnhuhbert_model = CNHubert(base_path, device=self.configs.device, dtype=torch.float16, state_dict=state_dict)
        self._hubert_state = state_dict
        self.configs.cnhuhbert_base_path = base_path

    def set_ref_audio(self, ref_audio_path: str):
        """reference TTS.py:737-747: prompt semantic tokens (HuBERT -> ssl_proj -> VQ) and the reference spectrogram."""
        self._set_prompt_semantic(ref_audio_path)
        self._set_ref_spec(ref_audio_path)
        self.prompt_cache["ref_audio_path"] = ref_audio_path

    def _ref_spec_or_handed(self, path: str, handed: Optional[dict]):
        """_get_ref_spec(path) and its speaker embedding (None: not computed yet), or, with `handed` (make_voices(shared_sv=True):
        path -> what _get_ref_spec returned and left in the prompt cache, plus the embedding of the shared pass), that entry"""
        if handed is None or path not in handed:
            return self._get_ref_spec(path), None
        h = handed[path]
        self.prompt_cache.update(raw_audio=h["raw_audio"], raw_sr=h["raw_sr"], ref_mel=None)
        return h["spec_audio"], h["sv_emb"]

    def _set_ref_spec(self, ref_audio_path: str, handed: Optional[dict] = None):
        spec_audio, emb = self._ref_spec_or_handed(ref_audio_path, handed)
        if self.prompt_cache["refer_spec"] in [[], None]:
            self.prompt_cache["refer_spec"] = [spec_audio]
        else:
            self.prompt_cache["refer_spec"][0] = spec_audio
        if spec_audio[1] is not None:
            # the reference recomputes the embedding inside every run() (TTS.py:1233-1238); it only depends on the reference audio
            if emb is None:
                emb = self.sv_model.compute_embedding3(spec_audio[1])
            cur = self.prompt_cache.get("sv_emb")
            if cur:
                cur[0] = emb
            else:
                self.prompt_cache["sv_emb"] = [emb]
        if self.vits_model is not None:
            self.vits_model.invalidate_refer()

    def init_sv_model(self, state_dict=None, path: Optional[str] = None):
        """reference TTS.py:672-675 / sv.py:11-23: the ERes2NetV2 speaker-verification model of v2Pro / v2ProPlus"""
        from .. import sv
        if getattr(self, "sv_model", None) is not None and state_dict is None and path is None:
            return
        self.sv_model = sv.SV(self.configs.device, self.configs.is_half, state_dict=state_dict, path=path or sv.sv_path)

    def _get_ref_spec(self, ref_audio_path: str):
        """reference TTS.py:761-800: mono, resampled to the model rate, divided by min(2, peak) when the peak exceeds 1,
        spectrogram_torch(filter_length, hop_length, win_length, center=False)."""
        from ..audio_io import load_wav, resample
        from ..module.mel_processing import spectrogram_torch
        is_v2pro = getattr(self.vits_model, "is_v2pro", False) or self.configs.version in ("v2Pro", "v2ProPlus")
        if is_v2pro and getattr(self, "sv_model", None) is None:
            raise RuntimeError("v2Pro / v2ProPlus: init_sv_model() first (ERes2NetV2 speaker embedding, sv.py:11-32)")
        raw, raw_sr = load_wav(ref_audio_path)
        self.prompt_cache["raw_audio"] = raw                     # [channels, n] float32 at raw_sr (TTS.py:759-762), host side
        self.prompt_cache["raw_sr"] = raw_sr
        self.prompt_cache["ref_mel"] = None                      # v3 / v4: recomputed from raw_audio on first use
        if raw.shape[0] == 2:
            raw = raw.mean(0, keepdims=True)
        audio = torch.from_numpy(resample(raw[:1], raw_sr, self.configs.sampling_rate)).to(self.configs.device)
        maxx = float(audio.abs().max())
        if maxx > 1:
            audio = audio / min(2.0, maxx)
        spec = spectrogram_torch(audio, self.configs.filter_length, self.configs.sampling_rate, self.configs.hop_length,
                                 self.configs.win_length, center=False)
        if self.configs.is_half:
            spec = spec.half()
        audio16k = None
        if is_v2pro:                                             # TTS.py:790-793: the normalised audio again at 16 kHz for the SV model
            audio16k = torch.from_numpy(resample(audio.cpu().numpy(), self.configs.sampling_rate, 16000)).to(self.configs.device)
            if self.configs.is_half:
                audio16k = audio16k.half()
        return spec, audio16k

    def _prompt_wav16k(self, ref_wav_path: str) -> np.ndarray:
        """reference TTS.py:802-810: the prompt audio at 16 kHz (3..10 s or OSError) with 0.3 s of silence behind it"""
        from ..audio_io import load_wav, resample
        raw, raw_sr = load_wav(ref_wav_path)
        wav16k = resample(raw.mean(0), raw_sr, 16000)
        if wav16k.shape[0] > 160000 or wav16k.shape[0] < 48000:
            raise OSError("参考音频在3~10秒范围外，请更换！")
        zero_wav = np.zeros(int(self.configs.sampling_rate * 0.3), dtype=np.float32)
        return np.concatenate([wav16k, zero_wav])

    device_frontend_calls = 0            # _load_refs_device calls that reached the device, for tests and tools/voice_enrol_bench.py

    def _load_refs_device(self, paths: Sequence[str], prompt_paths: Optional[Sequence[str]] = None) -> Dict[str, dict]:
        """The reference-audio front-end of make_voices(device_frontend=True): what _prompt_wav16k and
        _get_ref_spec compute for every distinct path of `paths`, with the files read on the host, uploaded in ONE copy from one
        page-locked buffer, and resampled, normalised and framed on the device in packed launches (one
        gsv_op_resample_poly_seg per (input rate, target rate), one spectrogram_torch_segments).  `prompt_paths` (default: all):
        the paths whose 16 kHz prompt is wanted and whose length is checked (3..10 s or OSError); an auxiliary reference only needs
        its spectrogram.  A missing file (ValueError) and a prompt outside 3..10 s are raised before any device work.
        -> path -> dict(wav16k: 1-D fp32 device prompt + 0.3 s of zeros (None outside prompt_paths), audio: [1, n] fp32 at the model
        rate divided by min(2, peak) where peak > 1, audio16k: [1, n16] of the engine dtype on v2Pro / v2ProPlus else None,
        spec: [1, bins, T] of the engine dtype, raw_audio / raw_sr: the file as load_wav returned it, on the host)."""
        from .. import audio_io as A
        from ..module.mel_processing import spectrogram_torch_segments
        cfg = self.configs
        dev = torch.device(cfg.device)
        sr_model = int(cfg.sampling_rate)
        is_v2pro = getattr(self.vits_model, "is_v2pro", False) or cfg.version in ("v2Pro", "v2ProPlus")
        if is_v2pro and getattr(self, "sv_model", None) is None:
            raise RuntimeError("v2Pro / v2ProPlus: init_sv_model() first (ERes2NetV2 speaker embedding, sv.py:11-32)")
        paths = list(dict.fromkeys(paths))
        prompts = set(paths if prompt_paths is None else prompt_paths)
        tail = int(cfg.sampling_rate * 0.3)
        # ---- host: read every file, settle every length, raise every file error ----
        chunks: List[np.ndarray] = []                             # what is uploaded, back to back
        jobs = {"w16": [], "aud": []}                             # target -> (path, chunk index, rate of the chunk)
        raws = {}
        for path in paths:
            if not os.path.exists(path):
                raise ValueError(f"{path} not exists")
            raw, sr = A.load_wav(path)
            raws[path] = (raw, sr)
            spec_mono = raw.mean(0) if raw.shape[0] == 2 else raw[0]
            srcs = {"aud": spec_mono}
            if path in prompts:
                n16 = A.resampled_len(raw.shape[1], sr, 16000)
                if n16 > 160000 or n16 < 48000:
                    raise OSError("参考音频在3~10秒范围外，请更换！")
                srcs["w16"] = spec_mono if raw.shape[0] <= 2 else raw.mean(0)
            staged = {}
            for target, rate in (("w16", 16000), ("aud", sr_model)):
                if target not in srcs:
                    continue
                mono, r = srcs[target], sr
                if r != rate and not A.device_resample_supported(r, rate):
                    mono, r = A.resample(mono, r, rate), rate   # a pair the kernel refuses: this file's host resampler
                k = (id(mono), r) if r == sr else (target, r)
                if k not in staged:
                    staged[k] = len(chunks)
                    chunks.append(np.ascontiguousarray(mono, dtype=np.float32))
                jobs[target].append((path, staged[k], r))
        offs = np.concatenate([[0], np.cumsum([c.shape[0] for c in chunks])]).astype(np.int64)
        # ---- one page-locked buffer, one upload ----
        self.device_frontend_calls += 1
        with torch.cuda.device(dev):
            host = torch.empty(int(offs[-1]), dtype=torch.float32, pin_memory=True)
            hv = host.numpy()
            for c, o in zip(chunks, offs):
                hv[o:o + c.shape[0]] = c
            stream = host.to(dev, non_blocking=True)

            def run(job, target_rate, out, out_starts, peaks):
                """one launch per input rate of `job` into out at out_starts (by job index); a chunk at the target rate is copied"""
                for r, idx in A.group_by_rate([j[2] for j in job]).items():
                    st = [int(offs[job[i][1]]) for i in idx]
                    ln = [int(chunks[job[i][1]].shape[0]) for i in idx]
                    if r == target_rate:
                        for i, a, n in zip(idx, st, ln):
                            out[out_starts[i]:out_starts[i] + n].copy_(stream[a:a + n])
                            if peaks is not None:
                                peaks[i] = out[out_starts[i]:out_starts[i] + n].abs().max()
                        continue
                    order = sorted(range(len(idx)), key=lambda q: st[q])    # the op takes ascending ranges; so are out_starts
                    _, _, pk = A.resample_segments(stream, [st[q] for q in order], [ln[q] for q in order], r, target_rate, out=out,
                                                   out_starts=[out_starts[idx[q]] for q in order], peak=peaks is not None)
                    if peaks is not None and len(idx) == len(job):
                        peaks.copy_(pk)
                    elif peaks is not None:
                        peaks[torch.tensor([idx[q] for q in order], device=dev)] = pk

            # the prompts at 16 kHz, each followed by `tail` zeros
            res = {p: dict(wav16k=None, audio16k=None, raw_audio=raws[p][0], raw_sr=raws[p][1]) for p in paths}
            job = jobs["w16"]
            if job:
                m16 = [A.resampled_len(chunks[j[1]].shape[0], j[2], 16000) for j in job]
                starts = [0] * len(job)
                for i in range(1, len(job)):
                    starts[i] = starts[i - 1] + m16[i - 1] + tail
                w16 = torch.zeros(starts[-1] + m16[-1] + tail, dtype=torch.float32, device=dev)
                run(job, 16000, w16, starts, None)
                for j, a, m in zip(job, starts, m16):
                    res[j[0]]["wav16k"] = w16[a:a + m + tail]
            # the model-rate audios with their peaks, normalised on the device
            job = jobs["aud"]
            ms = [A.resampled_len(chunks[j[1]].shape[0], j[2], sr_model) for j in job]
            starts = [0] * len(job)
            for i in range(1, len(job)):
                starts[i] = starts[i - 1] + ms[i - 1]
            aud = torch.empty(sum(ms), dtype=torch.float32, device=dev)
            peaks = torch.zeros(len(job), dtype=torch.float32, device=dev)
            run(job, sr_model, aud, starts, peaks)
            aud = self._normalise_refs(aud, ms, peaks)
            specs = spectrogram_torch_segments(aud, starts, ms, cfg.filter_length, sr_model, cfg.hop_length, cfg.win_length)
            a16 = None
            if is_v2pro:                                          # the normalised audio again at 16 kHz for the SV model
                if sr_model == 16000:
                    a16, tab16 = aud, list(zip(starts, ms))
                elif A.device_resample_supported(sr_model, 16000):
                    a16, tab16, _ = A.resample_segments(aud, starts, ms, sr_model, 16000)
                else:
                    parts = [torch.from_numpy(A.resample(aud[a:a + m].cpu().numpy(), sr_model, 16000)).to(dev) for a, m in zip(starts, ms)]
                    a16, tab16, o = torch.cat(parts), [], 0
                    for p in parts:
                        tab16.append((o, int(p.numel())))
                        o += int(p.numel())
                if cfg.is_half:
                    a16 = a16.half()
            for i, (j, a, m) in enumerate(zip(job, starts, ms)):
                r = res[j[0]]
                r["audio"] = aud[a:a + m].unsqueeze(0)
                r["spec"] = specs[i].half() if cfg.is_half else specs[i]
                if a16 is not None:
                    r["audio16k"] = a16[tab16[i][0]:tab16[i][0] + tab16[i][1]].unsqueeze(0)
        return res

    @staticmethod
    def _normalise_refs(aud: torch.Tensor, lens: Sequence[int], peaks: torch.Tensor) -> torch.Tensor:
        """_get_ref_spec's `audio / min(2, peak)` where peak > 1, for the audios of `lens` samples back to back in `aud`, from their
        device peaks: no readback.  Dividing by 1 leaves the other audios' bits as they are."""
        div = torch.where(peaks > 1, peaks.clamp(max=2.0), torch.ones_like(peaks))
        reps = torch.tensor(list(lens), dtype=torch.int64).to(aud.device, non_blocking=True)
        return aud / torch.repeat_interleave(div, reps, output_size=int(sum(lens)))

    def _device_refs(self, missing, shared_sv: bool) -> Tuple[Dict[str, dict], Dict[str, torch.Tensor]]:
        """make_voices(device_frontend=True): one _load_refs_device over every distinct main and auxiliary reference of the
        `missing` voice keys -> (handed: path -> dict(spec_audio, raw_audio, raw_sr, sv_emb) for _ref_spec_or_handed, sv_emb None
        unless shared_sv on a model with speaker embeddings; wav16k: main path -> the device prompt)"""
        mains = list(dict.fromkeys(key[0] for key in missing))
        for path in mains:                                        # the main references first: theirs are the errors make_voices raises
            if not os.path.exists(path):
                raise ValueError(f"{path} not exists")
        paths = list(mains)
        for key in missing:
            for path in key[3]:
                if path not in [None, ""] and os.path.exists(path) and path not in paths:
                    paths.append(path)
        refs = self._load_refs_device(paths, prompt_paths=mains)
        handed = {p: dict(spec_audio=(r["spec"], r["audio16k"]), raw_audio=r["raw_audio"], raw_sr=r["raw_sr"], sv_emb=None)
                  for p, r in refs.items()}
        if shared_sv and all(r["audio16k"] is not None for r in refs.values()):
            for path, emb in zip(paths, self.sv_model.compute_embedding3_many([refs[p]["audio16k"] for p in paths])):
                handed[path]["sv_emb"] = emb
        return handed, {p: refs[p]["wav16k"] for p in mains}

    def _set_prompt_semantic(self, ref_wav_path: str, hubert_feature: Optional[torch.Tensor] = None,
                             codes: Optional[torch.Tensor] = None, wav16k: Optional[np.ndarray] = None):
        """reference TTS.py:802-819: 16 kHz audio (3..10 s or OSError) + 0.3 s of silence -> HuBERT last_hidden_state ->
        SynthesizerTrn.extract_latent codes.  `hubert_feature` [1, 768, T50]: HuBERT is skipped; `codes` [1, 1, T50 // 2]:
        extract_latent too (make_voices computes both for many voices at once); `wav16k`: what _prompt_wav16k returned for
        this path, so that the file is not read again."""
        if getattr(self, "cnhuhbert_model", None) is None:
            raise RuntimeError("init_cnhuhbert_weights() first")
        if self.vits_model is None:
            raise RuntimeError("init_vits_weights() first")
        if wav16k is None:
            wav16k = self._prompt_wav16k(ref_wav_path)
        if codes is None:
            if hubert_feature is None:
                wav = torch.from_numpy(wav16k).to(self.configs.device)
                hubert_feature = self.cnhuhbert_model.model(wav.unsqueeze(0))["last_hidden_state"].transpose(1, 2)
            codes = self.vits_model.extract_latent(hubert_feature)
        self.prompt_cache["prompt_semantic"] = codes[0, 0].to(self.configs.device)

    def stop(self):
        self.stop_flag = True

    # ---- batching (reference TTS.py:842-973) ------------------------------------------------
    def to_batch(self, data: list, prompt_data: Optional[dict] = None, batch_size: int = 5, threshold: float = 0.75,
                 split_bucket: bool = True, device=torch.device("cpu"), precision=torch.float32):
        """Length-sorted bucketing: a candidate bucket [pos, pos_end) is accepted when its median /
        mean text length ratio reaches `threshold` (or it is a single item), otherwise it shrinks from
        the long end (TTS.py:859-879).  Items then get prompt phones / bert prepended (:899-904)."""
        lens = [len(it["norm_text"]) for it in data]
        batch_index_list: List[List[int]] = []
        if split_bucket:
            order = sorted(range(len(data)), key=lambda i: lens[i])       # stable, like list.sort
            sl = np.array([lens[i] for i in order], dtype=np.float32)
            pos = 0
            while pos < len(order):
                end = min(pos + batch_size, len(order))
                while True:
                    seg = sl[pos:end]
                    score = seg[(end - pos) // 2] / (seg.mean() + 1e-8)
                    if score >= threshold or end - pos == 1:
                        break
                    end -= 1
                batch_index_list.append([order[i] for i in range(pos, end)])
                pos = end
            assert sum(len(b) for b in batch_index_list) == len(data)
        else:
            for i in range(len(data)):
                if i % batch_size == 0:
                    batch_index_list.append([])
                batch_index_list[-1].append(i)
        batches = []
        zero_cache: Dict[int, bool] = {}

        def is_zero(t: Optional[torch.Tensor]) -> bool:
            # all-zero BERT features (every non-zh segment, TextPreprocessor.py:216-220) are passed to the
            # engine as None: bert_proj(0) is its bias, so the [1024, X] tensor never has to reach HBM
            if t is None:
                return True
            k = id(t)
            if k not in zero_cache:
                # host tensors: numpy is ~10x cheaper than a torch dispatch per segment, and an integer max over the bit patterns
                # 3x cheaper than any() (5.5 vs 16.6 us per 330 KB block; -0.0 counts as non-zero, which only forgoes the shortcut)
                if t.device.type == "cpu" and not t.requires_grad and t.dtype == torch.float32 and t.is_contiguous():
                    zero_cache[k] = t.numel() == 0 or int(t.numpy().view(np.uint32).max()) == 0
                elif t.device.type == "cpu" and not t.requires_grad:
                    zero_cache[k] = not t.numpy().any()
                else:
                    zero_cache[k] = not bool(torch.any(t))
            return zero_cache[k]

        for index_list in batch_index_list:
            phones_list, phones_len, all_phones, all_len, all_bert, texts, w2p = [], [], [], [], [], [], []
            max_len = 0
            for idx in index_list:
                it = data[idx]
                ph = torch.LongTensor(it["phones"]).to(device)
                if prompt_data is not None:
                    ap = torch.LongTensor(list(prompt_data["phones"]) + list(it["phones"])).to(device)
                    nb = (prompt_data["bert_features"].shape[-1] if prompt_data["bert_features"] is not None
                          else len(prompt_data["phones"])) + \
                         (it["bert_features"].shape[-1] if it["bert_features"] is not None else len(it["phones"]))
                    if is_zero(prompt_data["bert_features"]) and is_zero(it["bert_features"]):
                        ab = None
                    else:
                        pb = prompt_data["bert_features"]
                        pb = torch.zeros(1024, len(prompt_data["phones"])) if pb is None else pb
                        ib = it["bert_features"]
                        ib = torch.zeros(1024, len(it["phones"])) if ib is None else ib
                        ab = torch.cat([pb, ib], 1).to(dtype=precision, device=device)
                else:
                    ap = ph
                    nb = it["bert_features"].shape[-1] if it["bert_features"] is not None else len(it["phones"])
                    ab = None if is_zero(it["bert_features"]) else it["bert_features"].to(dtype=precision, device=device)
                max_len = max(max_len, nb, ap.shape[-1])
                phones_list.append(ph)
                phones_len.append(ph.shape[-1])
                all_phones.append(ap)
                all_len.append(ap.shape[-1])
                all_bert.append(ab)
                texts.append(it["norm_text"])
                w2p.append(it.get("word2ph"))
            batches.append({
                "phones": phones_list, "phones_len": torch.LongTensor(phones_len).to(device),
                "all_phones": all_phones, "all_phones_len": torch.LongTensor(all_len).to(device),
                "all_bert_features": all_bert, "norm_text": texts, "max_len": max_len,
                **({"word2ph": w2p} if any(w is not None for w in w2p) else {}),     # zh: phonemes per character (section 4w)
            })
        return batches, batch_index_list

    def recovery_order(self, data: list, batch_index_list: list) -> list:
        """put batch-ordered fragments back in submission order (TTS.py:957-973)."""
        n = sum(len(b) for b in batch_index_list)
        out = [None] * n
        for i, index_list in enumerate(batch_index_list):
            for j, index in enumerate(index_list):
                out[index] = data[i][j]
        return out

    def audio_postprocess(self, audio: List[List[torch.Tensor]], sr: int, batch_index_list: Optional[list] = None,
                          speed_factor: float = 1.0, split_bucket: bool = True, fragment_interval: float = 0.3,
                          super_sampling: bool = False, sample_rate: Optional[int] = None,
                          encoding: Optional[str] = None, loudness: Optional[float] = None, loudness_scope: str = "fragment",
                          loudness_peak: float = 0.0) -> Tuple[int, np.ndarray]:
        """TTS.py:1377-1429: per fragment divide by its peak if the peak exceeds 1, append
        int(sr*interval) zeros, restore order, concatenate, scale by 32768 and truncate to int16.

        super_sampling (TTS.py:1407-1417): the same concatenation as fp32 (gsv_postprocess_f32), AP_BWE to 48 kHz, then the
        peak rule and int16 step of gsv_postprocess on that one fragment without a gap; returns 48000.

        sample_rate / encoding (None: the launches above, unchanged): the same normalised concatenation
        resampled to `sample_rate` and written as int16 ("pcm_s16", saturating) or as G.711 bytes ("mulaw", "alaw") by one
        gsv_postprocess_groups_rate call -- the sentences in recovered order are one group; with super_sampling the 48 kHz
        AP_BWE result is the one sentence of a group without a gap -- and one copy; returns (sample_rate, int16 or uint8).

        loudness (None: everything above, unchanged): a target in LUFS.  The fragment (scope "fragment":
        the whole normalised concatenation, gaps included) or each of its sentences (scope "sentence") is metered after ITU-R
        BS.1770 on the device and multiplied by one gain towards the target, which loudness_peak (dBFS <= 0) caps at the
        peak.  Such a call always leaves through gsv_postprocess_groups_loud, with the identity filter when it names no other
        rate, so its int16 saturates instead of wrapping.  With super_sampling the 48 kHz AP_BWE result is the one sentence
        that is metered, at 48 kHz.  self.last_loudness becomes this call's reports, [[one record per span]]; it is
        replaced, never extended, so a server that calls this per request holds the last call's only (run() and run_batch()
        gather the reports of their own calls)."""
        import ctypes as C
        from .. import _lib
        dev = torch.device(self.configs.device)
        if dev.type != "cuda":
            raise RuntimeError("audio_postprocess is a HIP kernel (gsv_postprocess); there is no CPU path")
        gap = int(self.configs.sampling_rate * fragment_interval)
        loud = None if loudness is None else [(loudness, loudness_scope, loudness_peak)]
        flat = self.recovery_order(audio, batch_index_list) if split_bucket else [f for b in audio for f in b]
        flat = [f.to(dev, self.precision).contiguous().view(-1) for f in flat]
        lens = [int(f.shape[0]) for f in flat]
        self.last_fragment_lengths = [n + gap for n in lens]                                   # used by gsv.sharding
        # one launch (`gsv_postprocess`, csrc/sola.hip): peak, division, gaps, order and the int16 conversion -- the
        # reference loops over fragments on the host with a sync each (TTS.py:1391-1396); only int16 crosses PCIe
        code = _lib.GSV_F16 if self.precision == torch.float16 else _lib.GSV_F32
        with torch.cuda.device(dev):
            ptrs = (C.c_void_p * max(len(flat), 1))(*[f.data_ptr() for f in flat])
            arr = (C.c_int * max(len(flat), 1))(*lens)
            st = torch.cuda.current_stream(dev)
            if super_sampling:
                self.init_sr_model()
                wav = torch.empty(sum(lens) + gap * len(lens), dtype=torch.float32, device=dev)
                _lib.check(_lib.lib().gsv_postprocess_f32(ptrs, arr, len(flat), code, gap, wav.data_ptr(), C.c_void_p(st.cuda_stream)),
                           "gsv_postprocess_f32")
                hr = self.sr_model.forward_device(wav, sr)
                sr = self.sr_model.config["hr_sampling_rate"]
                if sample_rate is not None or encoding is not None or loudness is not None:
                    res = self._postprocess_rate([([hr.view(-1)], 0)], sr, sample_rate, encoding, loud)
                    self.last_loudness = res[3]
                    return res[:2]
                pcm = torch.empty(int(hr.shape[0]), dtype=torch.int16, device=dev)
                one_p, one_n = (C.c_void_p * 1)(hr.data_ptr()), (C.c_int * 1)(int(hr.shape[0]))
                _lib.check(_lib.lib().gsv_postprocess(one_p, one_n, 1, _lib.GSV_F32, 0, pcm.data_ptr(), C.c_void_p(st.cuda_stream)),
                           "gsv_postprocess")
                return sr, self._to_host(pcm)
            if sample_rate is not None or encoding is not None or loudness is not None:
                res = self._postprocess_rate([(flat, gap)], sr, sample_rate, encoding, loud)
                self.last_loudness = res[3]
                return res[:2]
            pcm = torch.empty(sum(lens) + gap * len(lens), dtype=torch.int16, device=dev)
            _lib.check(_lib.lib().gsv_postprocess(ptrs, arr, len(flat), code, gap, pcm.data_ptr(), C.c_void_p(st.cuda_stream)),
                       "gsv_postprocess")
        return sr, self._to_host(pcm)

    def _postprocess_rate(self, groups: Sequence[Tuple[Sequence[torch.Tensor], int]], sr: int, sample_rate: Optional[int],
                          encoding: Optional[str], loudness: Optional[Sequence[Optional[tuple]]] = None
                          ) -> Tuple[int, np.ndarray, List[int], list]:
        """One gsv_postprocess_groups_rate call (csrc/sola.hip) and one device-to-host copy: groups[g] =
        (its sentences, 1-D device tensors of one dtype, fp16 or fp32; its gap in samples at `sr`) -> (the output rate, all
        groups packed, int16 or uint8; the n_groups + 1 offsets of the groups in it).  sample_rate None is `sr` (the identity
        filter), encoding None is "pcm_s16".  The table and the workspace are the pipeline's, as in postprocess_fragments.
        loudness (None: that call exactly): per group None or (target LUFS, scope, peak dBFS).  A group with settings is one
        span with its gaps ("fragment") or one span per sentence ("sentence"), and the call is gsv_postprocess_groups_loud
        with `sr` as the metered rate; a group without settings has no span and keeps gain 1.  The
        report is copied to the host on the same stream in front of the audio and read after the one wait the audio needs.
        The fourth result lists, per group with settings, [{"lufs", "gain_db", "limited"} per span] (empty without `loudness`)."""
        import ctypes as C
        from .. import _lib, audio_io
        dev = torch.device(self.configs.device)
        sr_out = int(sr) if sample_rate is None else int(sample_rate)
        fmt = audio_io.ENCODINGS["pcm_s16" if encoding is None else encoding]
        if not audio_io.output_rate_supported(sr, sr_out):
            raise ValueError(f"sample_rate {sr_out}: the resampling kernel does not take {sr} -> {sr_out}")
        flat = [f for frags, _ in groups for f in frags]
        counts, gaps = [len(frags) for frags, _ in groups], [int(g) for _, g in groups]
        n, code = len(flat), _lib.dtype_code(flat[0].dtype if flat else self.precision)
        lens = (C.c_int * max(n, 1))(*[int(f.shape[0]) for f in flat])
        ptrs = (C.c_void_p * max(n, 1))(*[f.data_ptr() for f in flat])
        group_n, group_gap = (C.c_int * len(groups))(*counts), (C.c_int * len(groups))(*gaps)
        off = (C.c_longlong * (len(groups) + 1))()
        l = _lib.lib()
        spans, owner, first = [], [], 0                                 # owner[k]: the group of span k
        for g, (cnt, cfg) in enumerate(zip(counts, loudness if loudness is not None else [None] * len(groups))):
            if cfg is not None and cnt:
                target, scope, peak = cfg
                if scope not in audio_io.LOUDNESS_SCOPES:
                    raise ValueError(f"loudness_scope {scope!r}: one of {', '.join(audio_io.LOUDNESS_SCOPES)}")
                for f, c in ([(first, cnt)] if scope == "fragment" else [(first + i, 1) for i in range(cnt)]):
                    spans.append(_lib.LoudSpan(f, c, int(scope == "fragment"), float(target), float(peak)))
                    owner.append(g)
            first += cnt
        if spans:
            span_arr = (_lib.LoudSpan * len(spans))(*spans)
            need = int(l.gsv_postprocess_groups_loud_workspace(lens, n, group_n, group_gap, len(groups), int(sr), len(spans)))
        else:
            need = int(l.gsv_postprocess_groups_rate_workspace(lens, n, len(groups)))
        if need < 0:
            raise RuntimeError(f"gsv_postprocess_groups_loud_workspace: bad lengths, counts or rate {int(sr)}" if spans else
                               "gsv_postprocess_groups_rate_workspace: bad lengths")
        with torch.cuda.device(dev):
            ws = getattr(self, "_post_groups_ws", None)
            if ws is None or ws[0].numel() < need:
                size = max(1 << 16, 2 * need)
                ws = self._post_groups_ws = (torch.empty(size, dtype=torch.uint8).pin_memory(),
                                             torch.empty(size, dtype=torch.uint8, device=dev))
            rs = getattr(self, "_post_loud_reports", None)               # the reports: kept like the workspace, grown on demand
            if spans and (rs is None or rs[0].numel() < 16 * len(spans)):
                size = max(1 << 12, 32 * len(spans))
                rs = self._post_loud_reports = (torch.empty(size, dtype=torch.uint8).pin_memory(),
                                                torch.empty(size, dtype=torch.uint8, device=dev))
            hd, up, down = audio_io.output_filter_device(sr, sr_out, dev)
            total = sum(audio_io.resampled_len(sum(int(f.shape[0]) for f in frags) + len(frags) * g, sr, sr_out)
                        for (frags, _), g in zip(groups, gaps))
            out = torch.empty(max(total, 1), dtype=torch.int16 if fmt == _lib.GSV_OUT_S16 else torch.uint8, device=dev)
            st = torch.cuda.current_stream(dev)
            rep_host = None
            if spans:
                rep_host, rep_dev = rs[0][:16 * len(spans)], rs[1][:16 * len(spans)]
                _lib.check(l.gsv_postprocess_groups_loud(ptrs, lens, n, code, group_n, group_gap, len(groups), out.data_ptr(), off,
                                                         ws[0].data_ptr(), ws[1].data_ptr(), hd.data_ptr(), int(hd.numel()), up, down,
                                                         fmt, int(sr), span_arr, len(spans), rep_dev.data_ptr(),
                                                         C.c_void_p(st.cuda_stream)), "gsv_postprocess_groups_loud")
                rep_host.copy_(rep_dev, non_blocking=True)              # in front of the audio: the wait below covers both
            else:
                _lib.check(l.gsv_postprocess_groups_rate(ptrs, lens, n, code, group_n, group_gap, len(groups), out.data_ptr(), off,
                                                         ws[0].data_ptr(), ws[1].data_ptr(), hd.data_ptr(), int(hd.numel()), up, down,
                                                         fmt, C.c_void_p(st.cuda_stream)), "gsv_postprocess_groups_rate")
            host = self._to_host(out)                                   # waits for the stream: `flat` and the table are done with
        assert int(off[len(groups)]) == total
        reports: list = []
        if loudness is not None:
            per_group: Dict[int, list] = {g: [] for g, cfg in enumerate(loudness) if cfg is not None}
            if rep_host is not None:
                for g, r in zip(owner, rep_host.numpy().view(_lib.LOUD_REPORT_DTYPE)):
                    gain = float(r["gain"])
                    per_group[g].append({"lufs": float(r["lufs"]), "gain_db": 20.0 * math.log10(gain) if gain > 0 else -math.inf,
                                         "gain": gain, "limited": bool(int(r["flags"]) & _lib.LOUD_LIMITED)})
            reports = [per_group[g] for g in sorted(per_group)]
        return sr_out, host[:total], [int(v) for v in off], reports

    def postprocess_fragments(self, groups: Sequence[Tuple[Sequence[torch.Tensor], float]], sample_rate: Optional[int] = None,
                              encoding: Optional[str] = None, loudness: Optional[Sequence[Optional[tuple]]] = None
                              ) -> List[np.ndarray]:
        """audio_postprocess([frags], sr, None, speed, False, fragment_interval) of several fragments in ONE launch pair and
        ONE device-to-host copy (`gsv_postprocess_groups`, csrc/sola.hip): groups[g] = (the sentences of one fragment, its
        fragment_interval) -> the int16 audio of each, what audio_postprocess returns for it alone (super_sampling is not
        handled here: AP-BWE runs per fragment).  The table and the workspace are kept on the pipeline and grow on demand;
        the call waits for its copy, so the next call may rewrite them.
        sample_rate / encoding (None: the launches above, unchanged): every fragment at that rate and in that encoding, as
        audio_postprocess gives it with the same keywords, from ONE gsv_postprocess_groups_rate call; int16 or uint8.
        loudness (None, or all None: as above): per fragment None or (target LUFS, scope, peak dBFS), the loudness keywords of
        audio_postprocess.  Fragments with and without settings, and with different ones, share the one call, which is then
        gsv_postprocess_groups_loud: its int16 saturates, also for the fragments without settings in it (+1.0 gives 32767
        where the launches above wrap to -32768).  self.last_loudness becomes the reports of the fragments with settings, in
        order."""
        import ctypes as C
        from .. import _lib
        dev = torch.device(self.configs.device)
        if dev.type != "cuda":
            raise RuntimeError("postprocess_fragments is a HIP kernel (gsv_postprocess_groups); there is no CPU path")
        if not groups:
            return []
        if loudness is not None and all(c is None for c in loudness):
            loudness = None
        if sample_rate is not None or encoding is not None or loudness is not None:
            rated = [([f.to(dev, self.precision).contiguous().view(-1) for f in frags], int(self.configs.sampling_rate * interval))
                     for frags, interval in groups]
            _, host, off, reports = self._postprocess_rate(rated, self._output_sr(), sample_rate, encoding, loudness)
            if loudness is not None:
                self.last_loudness = reports
            return [host[off[g]:off[g + 1]].copy() for g in range(len(groups))]
        flat = [f.to(dev, self.precision).contiguous().view(-1) for frags, _ in groups for f in frags]
        gaps = [int(self.configs.sampling_rate * interval) for _, interval in groups]
        counts = [len(frags) for frags, _ in groups]
        n, code = len(flat), _lib.GSV_F16 if self.precision == torch.float16 else _lib.GSV_F32
        lens = (C.c_int * max(n, 1))(*[int(f.shape[0]) for f in flat])
        ptrs = (C.c_void_p * max(n, 1))(*[f.data_ptr() for f in flat])
        group_n, group_gap = (C.c_int * len(groups))(*counts), (C.c_int * len(groups))(*gaps)
        off = (C.c_longlong * (len(groups) + 1))()
        l = _lib.lib()
        need = int(l.gsv_postprocess_groups_workspace(lens, n))
        if need < 0:
            raise RuntimeError("gsv_postprocess_groups_workspace: bad lengths")
        with torch.cuda.device(dev):
            ws = getattr(self, "_post_groups_ws", None)
            if ws is None or ws[0].numel() < need:
                size = max(1 << 16, 2 * need)
                ws = self._post_groups_ws = (torch.empty(size, dtype=torch.uint8).pin_memory(),
                                             torch.empty(size, dtype=torch.uint8, device=dev))
            total = sum(int(f.shape[0]) for f in flat) + sum(c * g for c, g in zip(counts, gaps))
            pcm = torch.empty(max(total, 1), dtype=torch.int16, device=dev)
            st = torch.cuda.current_stream(dev)
            _lib.check(l.gsv_postprocess_groups(ptrs, lens, n, code, group_n, group_gap, len(groups), pcm.data_ptr(), off,
                                                ws[0].data_ptr(), ws[1].data_ptr(), C.c_void_p(st.cuda_stream)), "gsv_postprocess_groups")
            host = self._to_host(pcm)                                   # waits for the stream: `flat` and the table are done with
        assert int(off[len(groups)]) == total
        return [host[int(off[g]):int(off[g + 1])].copy() for g in range(len(groups))]

    def _to_host(self, t: torch.Tensor) -> np.ndarray:
        from gsv.hostcopy import to_host
        return to_host(t)

    # ---- v3 / v4 synthesis (reference TTS.py:1431-1637) -----------------------------------------
    def _prompt_features(self, lora_voice: Optional[str] = None):
        """... `lora_voice`: the encoder-side engine of that LoRA voice computes fea_ref and holds the style vector"""
        enc_model = self.vits_model if lora_voice is None else self._lora_voice(lora_voice)[0]
        pc = self.prompt_cache
        if pc.get("ref_mel") is None and pc.get("raw_audio") is not None:
            pc["ref_mel"] = self._ref_mel_from_audio(pc["raw_audio"], pc["raw_sr"])
        if pc.get("ref_mel") is None or pc["phones"] is None:
            raise NO_PROMPT_ERROR("v3/v4 need set_ref_audio(path) or set_prompt_cache(..., phones=..., ref_mel=...)")
        dev = self.configs.device
        spec = pc["refer_spec"][0]
        spec = spec[0] if isinstance(spec, tuple) else spec
        spec = spec.to(dev)
        fea_ref, ge = enc_model.decode_encp(pc["prompt_semantic"].view(1, 1, -1), torch.as_tensor(pc["phones"]).view(1, -1), spec)
        mel2 = norm_spec(pc["ref_mel"].to(dev, torch.float32))
        T_min = min(mel2.shape[2], fea_ref.shape[2])
        mel2, fea_ref = mel2[:, :, :T_min], fea_ref[:, :, :T_min]
        T_ref = self.vocoder_configs["T_ref"]
        if T_min > T_ref:
            mel2, fea_ref, T_min = mel2[:, :, -T_ref:], fea_ref[:, :, -T_ref:], T_ref
        return spec, fea_ref, ge, mel2.to(self.precision), T_min

    def _ref_mel_from_audio(self, raw_audio: np.ndarray, raw_sr: int) -> torch.Tensor:
        """TTS.py:1442-1453 / 1512-1523: mono mix of a stereo file, resampled to the vocoder's rate (24 kHz v3, 32 kHz v4),
        `mel_fn` / `mel_fn_v4` -> [1, 100, frames] (un-normalised: `_prompt_features` applies norm_spec)."""
        from ..audio_io import resample
        audio = np.asarray(raw_audio, dtype=np.float32)
        if audio.ndim == 1:
            audio = audio[None]
        if audio.shape[0] == 2:
            audio = audio.mean(0, keepdims=True)
        tgt_sr = 24000 if self.configs.version == "v3" else 32000
        audio = torch.from_numpy(resample(audio[:1], raw_sr, tgt_sr)).to(self.configs.device)
        return (mel_fn if self.configs.version == "v3" else mel_fn_v4)(audio)

    @torch.no_grad()
    def using_vocoder_synthesis(self, semantic_tokens: torch.Tensor, phones: torch.Tensor, speed: float = 1.0,
                                sample_steps: int = 32, seed: int = 0, noise_fn: Optional[Callable] = None,
                                inference_cfg_rate: float = 0, lora_voice: Optional[str] = None,
                                align_out: Optional[list] = None) -> torch.Tensor:
        """TTS.py:1431-1494: one fragment; the mel is generated chunk by chunk, each chunk prompted with the tail of the
        previous one.  `noise_fn(call_index, shape)` (tests) pins the randn draw of each cfm.inference call.
        `inference_cfg_rate` is CFM.inference_guided's (the reference passes 0 here: CFM.inference).  `lora_voice`: a name
        given to add_lora_voice; its encoder-side engine and its adapters in the DiT replace the base model's."""
        enc_model, slot = (self.vits_model, None) if lora_voice is None else self._lora_voice(lora_voice)
        lora_kw = {} if slot is None else dict(adapters=[slot])
        spec, fea_ref, ge, mel2, T_min = self._prompt_features(lora_voice)
        chunk_len = self.vocoder_configs["T_chunk"] - T_min
        # align_out (a list): the sentence's phoneme alignment (frames, ends, score) is appended to it
        fea_todo, ge = enc_model.decode_encp(semantic_tokens, phones, spec, ge, speed, **({} if align_out is None else {"align": True}))
        if align_out is not None:
            align_out.append((2 * int(semantic_tokens.shape[-1]),) + enc_model.last_alignment[0])
        outs, pos, call = [], 0, 0
        while True:
            chunk = fea_todo[:, :, pos:pos + chunk_len]
            if chunk.shape[-1] == 0:
                break
            pos += chunk_len
            fea = torch.cat([fea_ref, chunk], 2).transpose(2, 1)
            nz = noise_fn(call, (1, 100, fea.shape[1])) if noise_fn else None
            res = self.vits_model.cfm.inference_guided(fea, None, mel2, sample_steps, inference_cfg_rate=inference_cfg_rate,
                                                       noise=nz, seed=seed + call, **lora_kw)
            res = res[:, :, mel2.shape[2]:]
            call += 1
            mel2 = res[:, :, -T_min:]
            fea_ref = chunk[:, :, -T_min:]
            outs.append(res)
        return self.vocoder(denorm_spec(torch.cat(outs, 2)))[0][0]

    @torch.no_grad()
    def using_vocoder_synthesis_batched_infer(self, idx_list: List[int], semantic_tokens_list: List[torch.Tensor],
                                              batch_phones: List[torch.Tensor], speed: float = 1.0, sample_steps: int = 32,
                                              seed: int = 0, noise_fn: Optional[Callable] = None,
                                              inference_cfg_rate: float = 0, lora_voice: Optional[str] = None,
                                              align_out: Optional[list] = None) -> List[torch.Tensor]:
        """TTS.py:1496-1609: all fragments of a batch concatenated, cut into overlapping chunks that go through ONE
        batched cfm.inference, vocoded as one sequence, re-joined with SOLA and split back per fragment.  `lora_voice` as in
        using_vocoder_synthesis: every row of the pass takes its adapter."""
        slot = None if lora_voice is None else self._lora_voice(lora_voice)[1]
        prompt = self._prompt_features(lora_voice)
        fea, lens, pad_len = self._fold_chunks(prompt, idx_list, semantic_tokens_list, batch_phones, speed, lora_voice, align_out)
        mel2 = prompt[3]
        nz = noise_fn(0, (fea.shape[0], 100, fea.shape[1])) if noise_fn else None
        lora_kw = {} if slot is None else dict(adapters=[slot] * int(fea.shape[0]))
        pred = self.vits_model.cfm.inference_guided(fea, None, mel2, sample_steps, inference_cfg_rate=inference_cfg_rate, noise=nz,
                                                    seed=seed, **lora_kw)
        return self._fold_audio(pred[:, :, mel2.shape[2]:], lens, pad_len)

    @staticmethod
    def _chunk_cuts(frames: int, chunk_len: int, ov: int) -> List[Tuple[int, int]]:
        """TTS.py:1553-1570 as arithmetic: the [start, stop) cuts of a fold of `frames` feature frames after `ov` frames of
        left padding, every cut starting `ov` before the previous one's end; the last one is padded to chunk_len"""
        cuts, pos, total = [], 0, frames + ov
        while True:
            if pos != 0:
                pos -= ov
            if pos >= total:
                return cuts
            cuts.append((pos, min(pos + chunk_len, total)))
            pos += chunk_len

    def _fold_chunks(self, prompt: tuple, idx_list: List[int], semantic_tokens_list: List[torch.Tensor],
                     batch_phones: List[torch.Tensor], speed: float,
                     lora_voice: Optional[str] = None, align_out: Optional[list] = None) -> Tuple[torch.Tensor, List[int], int]:
        """the CFM input rows of one fold with the voice of `prompt` (= _prompt_features(lora_voice)): [chunks, T_chunk, 512],
        every row the voice's fea_ref followed by one chunk; the sentences' frame counts; the padding of the last chunk"""
        enc_model = self.vits_model if lora_voice is None else self._lora_voice(lora_voice)[0]
        spec, fea_ref, ge, mel2, T_min = prompt
        vc = self.vocoder_configs
        chunk_len, ov = vc["T_chunk"] - T_min, vc["overlapped_len"]
        feats, lens = [], []
        for i, idx in enumerate(idx_list):
            f, _ = enc_model.decode_encp(semantic_tokens_list[i][-idx:].view(1, 1, -1), batch_phones[i].view(1, -1), spec, ge, speed,
                                         **({} if align_out is None else {"align": True}))
            if align_out is not None:          # as in using_vocoder_synthesis
                align_out.append((2 * int(idx),) + enc_model.last_alignment[0])
            feats.append(f)
            lens.append(int(f.shape[2]))
        padded = F.pad(torch.cat(feats, 2), (ov, 0))
        chunks, pad_len = [], 0
        for a, b in self._chunk_cuts(sum(lens), chunk_len, ov):
            chunk = padded[:, :, a:b]
            pad_len = chunk_len - chunk.shape[2]
            if pad_len:
                chunk = F.pad(chunk, (0, pad_len))
            chunks.append(chunk)
        chunks = torch.cat(chunks, 0)
        return torch.cat([fea_ref.repeat(chunks.shape[0], 1, 1), chunks], 2).transpose(2, 1), lens, pad_len

    def _fold_audio(self, pred: torch.Tensor, lens: List[int], pad_len: int) -> List[torch.Tensor]:
        """the generated frames [chunks, 100, chunk_len] of one fold -> its sentences' waveforms (TTS.py:1581-1609)"""
        audio = self.vocoder(self._fold_mel(pred))[0][0]
        return self._fold_tail(audio, int(pred.shape[2]), lens, pad_len)

    @staticmethod
    def _fold_mel(pred: torch.Tensor) -> torch.Tensor:
        """the generated frames [chunks, 100, chunk_len] of one fold as the one mel [1, 100, chunks * chunk_len] its vocoder
        call takes (TTS.py:1581-1583)"""
        return denorm_spec(pred.permute(1, 0, 2).contiguous().view(pred.shape[1], -1).unsqueeze(0))

    def _fold_tail(self, audio: torch.Tensor, chunk_len: int, lens: List[int], pad_len: int) -> List[torch.Tensor]:
        """the vocoded fold [chunks * chunk_len * upsample_rate] -> its sentences' waveforms: cut into the chunks' pieces, SOLA,
        trim, split per sentence (TTS.py:1585-1609)"""
        vc = self.vocoder_configs
        ov, up = vc["overlapped_len"], vc["upsample_rate"]
        pieces, p = [], 0
        while p < audio.shape[-1]:
            pieces.append(audio[p:p + chunk_len * up])
            p += chunk_len * up
        audio = self.sola_algorithm(pieces, ov * up)
        audio = audio[ov * up:-pad_len * up]      # as written in the reference (TTS.py:1600): empty when pad_len == 0
        out = []
        for n in lens:
            out.append(audio[:n * up])
            audio = audio[n * up:]
        return out

    def sola_algorithm(self, audio_fragments: List[torch.Tensor], overlap_len: int) -> torch.Tensor:
        """TTS.py:1611-1637 on the device (`gsv_sola`, csrc/sola.hip): correlation, argmax and cross-fade per
        neighbouring pair, then one compaction; only the stitched length returns to the host."""
        import ctypes as C
        from .. import _lib
        dev = self.configs.device
        dt = audio_fragments[0].dtype
        lens = [int(f.shape[0]) for f in audio_fragments]
        with torch.cuda.device(dev):
            buf = torch.cat([f.to(dev, torch.float32) for f in audio_fragments]).contiguous()
            out = torch.empty_like(buf)
            n_out = C.c_int(0)
            arr = (C.c_int * len(lens))(*lens)
            st = torch.cuda.current_stream(dev)
            _lib.check(_lib.lib().gsv_sola(buf.data_ptr(), arr, len(lens), int(overlap_len), out.data_ptr(), C.byref(n_out),
                                           C.c_void_p(st.cuda_stream)), "gsv_sola")
        return out[:n_out.value].to(dt)

    def _prepare_prompt(self, inputs: dict, handed: Optional[dict] = None) -> None:
        """run()'s reference-audio / prompt-text handling (reference TTS.py:1078-1120): brings self.prompt_cache up to date
        with the request's ref_audio_path, aux_ref_audio_paths and prompt_text / prompt_lang.  `handed`: spectrograms and
        speaker embeddings computed ahead for the auxiliary references (_ref_spec_or_handed)."""
        ref_audio_path = inputs.get("ref_audio_path")
        prompt_text, prompt_lang = inputs.get("prompt_text"), inputs.get("prompt_lang", "")
        if ref_audio_path in [None, ""] and inputs.get("segments") is None and "text" in inputs and (
                self.prompt_cache["prompt_semantic"] is None or self.prompt_cache["refer_spec"] in [None, []]):
            raise ValueError("ref_audio_path cannot be empty, when the reference audio is not set using set_ref_audio()")
        if ref_audio_path not in [None, ""] and ref_audio_path != self.prompt_cache["ref_audio_path"]:
            if not os.path.exists(ref_audio_path):
                raise ValueError(f"{ref_audio_path} not exists")
            self.set_ref_audio(ref_audio_path)
        # auxiliary references for multi-speaker tone fusion (reference TTS.py:1098-1113): their spectrograms (and, v2Pro,
        # speaker embeddings) follow the main one; the style vector is the mean over all of them (models.py:971-985)
        aux = inputs.get("aux_ref_audio_paths") or []
        cached = self.prompt_cache.get("aux_ref_audio_paths") or []
        if "aux_ref_audio_paths" in inputs and not (len(set(aux) & set(cached)) == len(aux) == len(cached)):
            if self.prompt_cache["refer_spec"] in [None, []]:
                raise ValueError("aux_ref_audio_paths need a main reference audio first (ref_audio_path / set_ref_audio)")
            self.prompt_cache["aux_ref_audio_paths"] = list(aux)
            self.prompt_cache["refer_spec"] = [self.prompt_cache["refer_spec"][0]]
            if self.prompt_cache.get("sv_emb"):
                self.prompt_cache["sv_emb"] = [self.prompt_cache["sv_emb"][0]]
            for path in aux:
                if path in [None, ""]:
                    continue
                if not os.path.exists(path):
                    print("音频文件不存在，跳过：", path)
                    continue
                spec_audio, emb = self._ref_spec_or_handed(path, handed)
                self.prompt_cache["refer_spec"].append(spec_audio)
                if spec_audio[1] is not None:
                    self.prompt_cache["sv_emb"].append(self.sv_model.compute_embedding3(spec_audio[1]) if emb is None else emb)
            self.vits_model.invalidate_refer()
        if prompt_text not in [None, ""]:
            from .text_segmentation_method import splits
            if prompt_lang not in self.configs.languages:
                raise ValueError(f"prompt_lang {prompt_lang!r} is not one of {self.configs.languages}")
            prompt_text = prompt_text.strip("\n")
            if prompt_text[-1] not in splits:
                prompt_text += "。" if prompt_lang != "en" else "."
            if self.prompt_cache["prompt_text"] != prompt_text:
                phones, bert_features, norm_text = self.text_preprocessor.segment_and_extract_feature_for_text(
                    prompt_text, prompt_lang, self.configs.version)
                self.prompt_cache.update(prompt_text=prompt_text, prompt_lang=prompt_lang, phones=phones,
                                         bert_features=bert_features, norm_text=norm_text)
        elif "prompt_text" in inputs and self.configs.use_vocoder:
            raise NO_PROMPT_ERROR("prompt_text cannot be empty when using SoVITS_V3")
        if not self.prompt_cache["refer_spec"] or (self.prompt_cache["prompt_semantic"] is None
                                                   and self.prompt_cache["phones"] is not None):
            raise NO_PROMPT_ERROR("set_prompt_cache() first (reference: ref_audio_path is required)")

    def _segments(self, inputs: dict) -> list:
        """run()'s text front-end (reference TTS.py:1018-1024, 1100-1135): the request's segments"""
        segments = inputs.get("segments")
        if segments is None:
            # reference TTS.py:1018-1024, 1100-1135: raw text through the TextPreprocessor (G2P back-ends are plug-ins,
            # gsv.text.cleaner.register_g2p); a `text_frontend` callable replaces it wholesale
            text, text_lang = inputs.get("text", ""), inputs.get("text_lang", "")
            method = inputs.get("text_split_method", "cut0")
            if self.text_frontend is not None:
                segments = self.text_frontend(text, text_lang, method)
            else:
                if text_lang not in self.configs.languages:
                    raise ValueError(f"text_lang {text_lang!r} is not one of {self.configs.languages}")
                if self.batched_bert:
                    segments = self.text_preprocessor.preprocess_many([(text, text_lang, method)], self.configs.version)[0]
                else:
                    segments = self.text_preprocessor.preprocess(text, text_lang, method, self.configs.version)
        return segments

    def _with_shared_segments(self, requests: List[dict]) -> List[dict]:
        """run_batch(shared_bert=True): the raw texts of all requests through ONE preprocess_many, each such request returned
        as a copy with its `segments` filled in.  Requests that bring `segments` pass through, and so does every request when a
        `text_frontend` replaces the preprocessor.  Raises what _segments raises for the request alone."""
        if self.text_frontend is not None:
            return list(requests)
        todo = [i for i, req in enumerate(requests) if req.get("segments") is None]
        for i in todo:
            if requests[i].get("text_lang", "") not in self.configs.languages:
                raise ValueError(f"text_lang {requests[i].get('text_lang', '')!r} is not one of {self.configs.languages}")
        items = [(requests[i].get("text", ""), requests[i].get("text_lang", ""), requests[i].get("text_split_method", "cut0"))
                 for i in todo]
        out = list(requests)
        for i, segments in zip(todo, self.text_preprocessor.preprocess_many(items, self.configs.version) if items else []):
            out[i] = dict(requests[i], segments=segments)
        return out

    def _voice_refer(self, voice: dict) -> Tuple[List[torch.Tensor], dict]:
        """the device reference of a voice or prompt-cache dict as SynthesizerTrn.decode takes it: (`refer`, the spectrograms
        on the device; `sv_kw`, the speaker embeddings as a keyword for v2Pro / v2ProPlus and nothing for the others)"""
        refer = [spec.to(device=self.configs.device) for spec, _ in voice["refer_spec"]]
        return refer, ({"sv_emb": voice["sv_emb"]} if getattr(self.vits_model, "is_v2pro", False) else {})

    @staticmethod
    def _kept_tokens(pred_list: List[torch.Tensor], idx_list: List[int], no_prompt: bool) -> Tuple[List[torch.Tensor], List[int]]:
        """The AR output of one to_batch batch without the prompts -> (`pred`, the generated tokens per sentence; the
        `idx_list` the waveform stage takes).  Prompt-free, y holds only generated tokens and idx is reported as 0
        (t2s_model.py:916-917): all are kept, idx_list becomes the lengths.  Else the last idx; 0 keeps none, not p[-0:]."""
        if no_prompt:
            pred = list(pred_list)
            return pred, [int(p.shape[0]) for p in pred]
        return [p[-i:] if i > 0 else p[:0] for p, i in zip(pred_list, idx_list)], idx_list

    def _decode_best_of(self, item: dict, prompt: torch.Tensor, o: dict, seed_b: int):
        """run()'s AR decode of one to_batch batch under "best_of" = n: every sentence n times, as n rows of the same
        prefill.  Sentence j has the key (seed_b, j mod max_batch) in the plain decode; candidate c draws with
        (seed_b, j mod max_batch + 1024 c), and each group of max_batch sentences keeps the step budget the plain decode
        gives it, so candidate 0 is the plain draw.  Returns (pred_list, idx_list) of the chosen candidates and the record of
        the choices per sentence (choose_candidate)."""
        t2s, n = self.t2s_model, o["best_of"]
        mb = t2s.max_batch
        x, bert = item["all_phones"], item["all_bert_features"]
        lens = [int(t.shape[-1]) for t in x]
        wanted = min(1500, int(early_stop_num(self.configs)) + 1)
        pred_list, idx_list, rec = [], [], []
        for lo in range(0, len(x), mb):
            js = [j for j in range(lo, min(lo + mb, len(x))) for _ in range(n)]
            budget = min(wanted, t2s.max_seq - (max(lens[lo:lo + mb]) + int(prompt.shape[1]) + 2))
            keys = [(seed_b, j % mb + BEST_OF_ROW_STRIDE * c) for j in range(lo, min(lo + mb, len(x))) for c in range(n)]
            ys, idx = t2s.infer_panel_batch_infer([x[j] for j in js], None, prompt[:1].expand(len(js), -1), [bert[j] for j in js],
                                                  top_k=o["top_k"], top_p=o["top_p"], temperature=o["temperature"],
                                                  early_stop_num=early_stop_num(self.configs),
                                                  repetition_penalty=o["repetition_penalty"], rng_keys=keys, max_steps=budget,
                                                  logprobs=True)
            lps, cuts = t2s.last_logprobs, t2s.last_cut
            for s0 in range(0, len(js), n):
                cands = [dict(tokens=ys[k][-idx[k]:] if idx[k] > 0 else ys[k][:0], logprobs=lps[k].cpu().numpy(), n=idx[k],
                              cut=cuts[k]) for k in range(s0, s0 + n)]
                k, r = choose_candidate(o, cands)
                pred_list.append(ys[s0 + k])
                idx_list.append(idx[s0 + k])
                rec.append(r)
        return pred_list, idx_list, rec

    def _synthesize_batch(self, item: dict, pred: List[torch.Tensor], pred_list: List[torch.Tensor], idx_list: List[int],
                          bi: int, actual_seed: int, opts: dict, voice_refer: Tuple[List[torch.Tensor], dict],
                          have: Optional[List[Optional[torch.Tensor]]] = None,
                          align_out: Optional[list] = None) -> List[torch.Tensor]:
        """run()'s post-AR stage of one to_batch batch `bi` (reference TTS.py:1259-1299): the fragments of its sentences from
        the generated tokens (`pred`, `idx_list` = _kept_tokens(`pred_list`, ...)), with the voice of self.prompt_cache
        (v3/v4) / `voice_refer` = _voice_refer(voice) (v1/v2/v2Pro), speed_factor, parallel_infer, sample_steps and
        inference_cfg_rate (v3/v4 only) of the resolved `opts`, and the seed actual_seed + bi.  `have` (v1/v2/v2Pro at
        speed_factor != 1 only): the sentences a shared pass already decoded, None where it left one out.  `align_out` (a list;
        "timestamps": "phone"): one (frames, ends, score) per sentence is appended, the phoneme alignment
        the SoVITS engine computes in the same pass; the audio does not depend on it."""
        speed_factor, seed_b = opts["speed_factor"], actual_seed + bi
        al_kw = {} if align_out is None else {"align_out": align_out}
        refer, sv_kw = voice_refer
        frags: List[torch.Tensor] = []
        if self.configs.use_vocoder:                                    # TTS.py:1283-1299
            dev_ph = [ph.to(self.configs.device) for ph in item["phones"]]
            cfm_kw = dict(speed=speed_factor, sample_steps=opts["sample_steps"], inference_cfg_rate=opts["inference_cfg_rate"])
            if opts.get("lora_voice") is not None:
                cfm_kw["lora_voice"] = opts["lora_voice"]
            if opts["parallel_infer"]:
                frags = self.using_vocoder_synthesis_batched_infer(idx_list, pred_list, dev_ph, seed=seed_b, **cfm_kw, **al_kw)
            else:
                for k, idx in enumerate(idx_list):
                    frags.append(self.using_vocoder_synthesis(pred_list[k][-idx:].view(1, 1, -1), dev_ph[k].view(1, -1),
                                                              seed=actual_seed + bi * 4096 + k, **cfm_kw, **al_kw))
        elif speed_factor == 1.0:
            # one decode over the batch folded into the time axis (TTS.py:1259-1282)
            cut = [int(p.shape[0]) * 2 * math.prod(self.vits_model.upsample_rates) for p in pred]
            keep = [k for k, p in enumerate(pred) if p.shape[0] > 0]
            if keep:
                all_pred = torch.cat([pred[k] for k in keep]).view(1, 1, -1)
                all_ph = torch.cat([item["phones"][k] for k in keep]).view(1, -1)
                spans, c0, p0 = [], 0, 0       # the fold's sentences back to back: one alignment span each
                for k in keep:
                    spans.append((c0, int(pred[k].shape[0]), p0, int(item["phones"][k].shape[0])))
                    c0, p0 = c0 + spans[-1][1], p0 + spans[-1][3]
                wav = self.vits_model.decode(all_pred, all_ph, refer, speed=speed_factor, seed=seed_b, **sv_kw,
                                             **({} if align_out is None else {"align": spans}))[0, 0]
            else:
                wav = torch.zeros(0, dtype=self.precision, device=self.configs.device)
            if align_out is not None:
                got = iter(self.vits_model.last_alignment if keep else [])
                for k, p in enumerate(pred):   # a sentence without tokens: no frames, every phoneme empty
                    align_out.append((2 * int(p.shape[0]),) + (next(got) if k in keep else
                                                               (np.zeros(int(item["phones"][k].shape[0]), np.int32), float("-inf"))))
            frags = list(torch.split(wav, cut))        # decode gives exactly 2 * up samples per token at speed 1
        else:
            for k, p in enumerate(pred):
                if have is not None and have[k] is not None:
                    frags.append(have[k])
                    if align_out is not None:
                        align_out.append(None)          # the shared pass that decoded it holds its alignment
                    continue
                frags.append(self.vits_model.decode(p.view(1, 1, -1), item["phones"][k].view(1, -1), refer,
                                                    speed=speed_factor, seed=seed_b, **sv_kw,
                                                    **({} if align_out is None else {"align": True}))[0, 0])
                if align_out is not None:
                    align_out.append((2 * int(p.shape[0]),) + self.vits_model.last_alignment[0])
        return frags

    # ---- several voices in one AR decode -----------------------------------------------------------
    _VOICE_KEYS = ("prompt_semantic", "refer_spec", "phones", "bert_features", "norm_text", "ref_mel", "sv_emb", "raw_audio",
                   "raw_sr", "ref_audio_path", "aux_ref_audio_paths", "prompt_text", "prompt_lang")

    @contextlib.contextmanager
    def _with_prompt_cache(self, cache: dict):
        """self.prompt_cache is `cache` inside the block and the caller's dict again after it; the SoVITS engine's cached
        reference terms (ge) are dropped on the way in and out, so no voice ever reuses another's style vector"""
        saved = self.prompt_cache
        self.prompt_cache = cache
        engines = [self.vits_model] + [v["engine"] for v in getattr(self, "_lora_voices", {}).values()]
        for e in engines:
            if e is not None:
                e.invalidate_refer()
        try:
            yield cache
        finally:
            self.prompt_cache = saved
            for e in engines:
                if e is not None:
                    e.invalidate_refer()

    def _empty_prompt_cache(self) -> dict:
        return {"ref_audio_path": None, "prompt_semantic": None, "refer_spec": [], "prompt_text": None, "prompt_lang": None,
                "phones": None, "bert_features": None, "norm_text": None, "aux_ref_audio_paths": [], "ref_mel": None,
                "sv_emb": None}

    def make_voice(self, prompt_semantic: Optional[torch.Tensor] = None, refer_spec: Optional[Sequence[torch.Tensor]] = None,
                   phones: Optional[List[int]] = None, bert_features: Optional[torch.Tensor] = None, norm_text: str = "",
                   ref_mel: Optional[torch.Tensor] = None, sv_emb: Optional[Sequence[torch.Tensor]] = None, *,
                   ref_audio_path: Optional[str] = None, prompt_text: Optional[str] = None, prompt_lang: str = "",
                   aux_ref_audio_paths: Optional[Sequence[str]] = None) -> dict:
        """A reference voice for run_batch: a snapshot of what set_prompt_cache (components: same arguments) or
        set_ref_audio + prompt text + aux_ref_audio_paths (keyword `ref_audio_path`, ...) store.  Voices made from audio are
        kept in a small LRU keyed by (ref_audio_path, prompt_text, prompt_lang, aux_ref_audio_paths).  self.prompt_cache is
        not changed."""
        if ref_audio_path is None:
            if prompt_semantic is None and phones is not None:
                raise NO_PROMPT_ERROR("a voice with prompt phones needs its prompt_semantic")
            with self._with_prompt_cache(self._empty_prompt_cache()) as pc:
                self.set_prompt_cache(prompt_semantic, refer_spec or [], phones=phones, bert_features=bert_features,
                                      norm_text=norm_text, ref_mel=ref_mel, sv_emb=sv_emb)
            return {k: pc.get(k) for k in self._VOICE_KEYS}
        key = (ref_audio_path, prompt_text, prompt_lang, tuple(aux_ref_audio_paths or ()))
        lru = self.__dict__.setdefault("_voice_lru", collections.OrderedDict())
        if key in lru:
            lru.move_to_end(key)
            return lru[key]
        req = {"ref_audio_path": ref_audio_path, "prompt_text": prompt_text, "prompt_lang": prompt_lang}
        if aux_ref_audio_paths is not None:
            req["aux_ref_audio_paths"] = list(aux_ref_audio_paths)
        with self._with_prompt_cache(self._empty_prompt_cache()) as pc:
            self._prepare_prompt(req)
        voice = {k: pc.get(k) for k in self._VOICE_KEYS}
        lru[key] = voice
        while len(lru) > self.voice_cache_size:
            lru.popitem(last=False)
        return voice

    voice_cache_size = 8

    def make_voices(self, specs: Sequence[dict], shared_sv: bool = False, device_frontend: bool = False) -> List[dict]:
        """make_voice(ref_audio_path=..., prompt_text=..., prompt_lang=..., aux_ref_audio_paths=...) for many specs (dicts of
        those keywords) with ONE packed HuBERT pass (HubertModel.batch) and one extract_latent_many over the reference audios
        that the voice LRU does not hold; every distinct ref_audio_path is loaded and encoded once.  The spectrogram, speaker
        embedding, auxiliary references and prompt text of each voice are computed by the code make_voice runs.  Returns one
        voice per spec, in order -- all of them, also when there are more than voice_cache_size; every new voice enters the
        LRU, which evicts as make_voice's does.  A missing file (ValueError) or a prompt outside 3..10 s (OSError) is raised
        before any device work.  self.prompt_cache is not changed.
        shared_sv=True (v2Pro / v2ProPlus; nothing changes on another model): the reference spectrograms of every distinct main
        and auxiliary path of the missing voices are computed first, then ONE SV.compute_embedding3_many runs over their 16 kHz
        audios (packed ERes2NetV2 passes) instead of one encoder pass per reference; the voices take their embeddings from it.
        device_frontend=True: the main and auxiliary references of the missing voices are read on the host, uploaded once, and
        resampled, normalised and framed on the device (_load_refs_device): HuBERT takes the device prompts, the spectrograms (and,
        with shared_sv, the embeddings) reach the voices as shared_sv's do.  The waveforms differ from the host resampler's by fp32
        rounding; errors, LRU and order are as above."""
        lru = self.__dict__.setdefault("_voice_lru", collections.OrderedDict())
        keys, out, missing = [], {}, []
        for spec in specs:
            unknown = set(spec) - {"ref_audio_path", "prompt_text", "prompt_lang", "aux_ref_audio_paths"}
            if unknown or spec.get("ref_audio_path") in [None, ""]:
                raise ValueError(f"make_voices: a spec takes ref_audio_path (required), prompt_text, prompt_lang and "
                                 f"aux_ref_audio_paths, got {sorted(spec)}")
            key = (spec["ref_audio_path"], spec.get("prompt_text"), spec.get("prompt_lang", ""),
                   tuple(spec.get("aux_ref_audio_paths") or ()))
            keys.append(key)
            if key in out or key in missing:
                continue
            if key in lru:
                lru.move_to_end(key)
                out[key] = lru[key]
            else:
                missing.append(key)
        if missing:
            if getattr(self, "cnhuhbert_model", None) is None:
                raise RuntimeError("init_cnhuhbert_weights() first")
            if self.vits_model is None:
                raise RuntimeError("init_vits_weights() first")
            wavs: Dict[str, Union[np.ndarray, torch.Tensor]] = {}
            handed = None
            if device_frontend:
                handed, wavs = self._device_refs(missing, shared_sv)
            for key in missing:                                   # host side first: every file error before any device work
                path = key[0]
                if path not in wavs:
                    if not os.path.exists(path):
                        raise ValueError(f"{path} not exists")
                    wavs[path] = self._prompt_wav16k(path)
            paths = list(wavs)
            feats = self.cnhuhbert_model.model.batch([wavs[p] if device_frontend else torch.from_numpy(wavs[p]) for p in paths])
            codes = dict(zip(paths, self.vits_model.extract_latent_many([f.transpose(1, 2) for f in feats])))
            spec_of = {key: spec for key, spec in zip(keys, specs)}
            if not device_frontend:
                handed = self._shared_sv_refs(missing) if shared_sv else None
            for key in missing:
                path, spec = key[0], spec_of[key]
                req = {"ref_audio_path": path, "prompt_text": spec.get("prompt_text"), "prompt_lang": spec.get("prompt_lang", "")}
                if spec.get("aux_ref_audio_paths") is not None:
                    req["aux_ref_audio_paths"] = list(spec["aux_ref_audio_paths"])
                with self._with_prompt_cache(self._empty_prompt_cache()) as pc:
                    # set_ref_audio with the codes handed in; _prepare_prompt then finds the path current and goes on to the
                    # auxiliary references and the prompt text
                    self._set_prompt_semantic(path, codes=codes[path], wav16k=wavs[path])
                    self._set_ref_spec(path, handed)
                    pc["ref_audio_path"] = path
                    self._prepare_prompt(req, handed)
                out[key] = lru[key] = {k: pc.get(k) for k in self._VOICE_KEYS}
                while len(lru) > self.voice_cache_size:
                    lru.popitem(last=False)
        return [out[key] for key in keys]

    def _shared_sv_refs(self, missing) -> Optional[dict]:
        """make_voices(shared_sv=True): path -> dict(spec_audio, raw_audio, raw_sr, sv_emb) for every distinct main and auxiliary
        reference of the `missing` voice keys that make_voice would read, the embeddings from one compute_embedding3_many;
        None on a model without speaker embeddings"""
        if not (getattr(self.vits_model, "is_v2pro", False) or self.configs.version in ("v2Pro", "v2ProPlus")):
            return None
        paths = []
        for key in missing:
            for path in (key[0],) + tuple(p for p in key[3] if p not in [None, ""] and os.path.exists(p)):
                if path not in paths:
                    paths.append(path)
        handed = {}
        for path in paths:
            with self._with_prompt_cache(self._empty_prompt_cache()) as pc:
                handed[path] = dict(spec_audio=self._get_ref_spec(path), raw_audio=pc["raw_audio"], raw_sr=pc["raw_sr"])
        embs = self.sv_model.compute_embedding3_many([handed[p]["spec_audio"][1] for p in paths])
        for path, emb in zip(paths, embs):
            handed[path]["sv_emb"] = emb
        return handed

    def _with_shared_voices(self, requests: List[dict], shared_sv: bool = False, device_frontend: bool = False) -> List[dict]:
        """run_batch(shared_hubert=True / shared_sv=True): the requests that name a ref_audio_path and bring no `voice` get
        theirs from ONE make_voices call, each returned as a copy with its `voice` filled in; the others pass through"""
        todo = [i for i, req in enumerate(requests) if req.get("voice") is None and req.get("ref_audio_path") not in [None, ""]]
        out = list(requests)
        if todo:
            specs = [{"ref_audio_path": requests[i]["ref_audio_path"], "prompt_text": requests[i].get("prompt_text"),
                      "prompt_lang": requests[i].get("prompt_lang", ""),
                      "aux_ref_audio_paths": requests[i].get("aux_ref_audio_paths")} for i in todo]
            for i, voice in zip(todo, self.make_voices(specs, shared_sv=shared_sv, device_frontend=device_frontend)):
                out[i] = dict(requests[i], voice=voice)
        return out

    def _request_voice(self, req: dict) -> dict:
        if req.get("voice") is not None:
            return req["voice"]
        if req.get("ref_audio_path") not in [None, ""]:
            return self.make_voice(ref_audio_path=req["ref_audio_path"], prompt_text=req.get("prompt_text"),
                                   prompt_lang=req.get("prompt_lang", ""), aux_ref_audio_paths=req.get("aux_ref_audio_paths"))
        if not self.prompt_cache["refer_spec"]:
            raise NO_PROMPT_ERROR("run_batch: a request without `voice` or `ref_audio_path` needs set_prompt_cache() first")
        return {k: self.prompt_cache.get(k) for k in self._VOICE_KEYS}

    @staticmethod
    def _request_options(req: dict) -> dict:
        """The keys run() accepts with the reference's defaults (TTS.py:1026-1046): the only place a request key is read
        with a default.  An empty seed is -1 (random) and fragment_interval is at least 0.01; `split_bucket` and
        `super_sampling` are as given -- _resolve_options applies the rules that depend on the loaded model.
        "lora_voice" (a name given to add_lora_voice) is carried only when the request names one: absent or None is the base
        model, and the options of such a request are the ones they were (read it with o.get("lora_voice")).  "best_of"
        (candidates per sentence) likewise only when the request names one other than 1, as given, with
        its "best_of_score" callable if it brings one: _resolve_options checks both.  "sample_rate" (int, Hz) and "encoding"
        ("pcm_s16", "mulaw", "alaw") are checked and carried only when the request gives them: a rate
        that is no positive int and an unknown encoding raise ValueError.  "loudness" (float, LUFS in -70 .. 0; DESIGN.md
        section 4v) brings "loudness_scope" ("fragment", the default, or "sentence") and "loudness_peak" (dBFS <= 0, default 0.0)
        with it; all three are carried only when the request gives "loudness", as floats (any real number, numpy's included,
        but no bool), and the other two without it, wrong types and values out of range raise ValueError."""
        o = dict(top_k=req.get("top_k", 5), top_p=req.get("top_p", 1), temperature=req.get("temperature", 1),
                 batch_size=req.get("batch_size", 1), batch_threshold=req.get("batch_threshold", 0.75),
                 speed_factor=req.get("speed_factor", 1.0), split_bucket=req.get("split_bucket", True),
                 return_fragment=req.get("return_fragment", False), fragment_interval=req.get("fragment_interval", 0.3),
                 parallel_infer=req.get("parallel_infer", True), repetition_penalty=req.get("repetition_penalty", 1.35),
                 sample_steps=req.get("sample_steps", 32), inference_cfg_rate=req.get("inference_cfg_rate", 0),
                 super_sampling=bool(req.get("super_sampling", False)))
        seed = req.get("seed", -1)
        o["seed"] = -1 if seed in ["", None] else seed
        if o["fragment_interval"] < 0.01:
            o["fragment_interval"] = 0.01
        if req.get("lora_voice") is not None:
            o["lora_voice"] = req["lora_voice"]
        n = req.get("best_of")
        if n is not None and not (type(n) is int and n == 1):
            o["best_of"] = n
            if req.get("best_of_score") is not None:
                o["best_of_score"] = req["best_of_score"]
        if req.get("sample_rate") is not None:
            rate = req["sample_rate"]
            if type(rate) is not int or rate <= 0:
                raise ValueError(f"sample_rate {rate!r}: a positive int, in Hz")
            o["sample_rate"] = rate
        if req.get("encoding") is not None:
            from ..audio_io import ENCODINGS
            if req["encoding"] not in ENCODINGS:
                raise ValueError(f"encoding {req['encoding']!r}: one of {', '.join(sorted(ENCODINGS))}")
            o["encoding"] = req["encoding"]
        if req.get("loudness") is not None:
            from ..audio_io import LOUDNESS_SCOPES
            target, scope, peak = req["loudness"], req.get("loudness_scope", "fragment"), req.get("loudness_peak", 0.0)
            real = lambda v: isinstance(v, numbers.Real) and not isinstance(v, (bool, np.bool_))     # noqa: E731
            if not real(target) or not -70.0 <= target <= 0.0:
                raise ValueError(f"loudness {target!r}: a target in LUFS, -70 <= v <= 0")
            if scope not in LOUDNESS_SCOPES:
                raise ValueError(f"loudness_scope {scope!r}: one of {', '.join(LOUDNESS_SCOPES)}")
            if not real(peak) or not peak <= 0.0:
                raise ValueError(f"loudness_peak {peak!r}: a ceiling in dBFS, at most 0")
            o["loudness"], o["loudness_scope"], o["loudness_peak"] = float(target), scope, float(peak)
        elif req.get("loudness_scope") is not None or req.get("loudness_peak") is not None:
            raise ValueError("loudness_scope / loudness_peak without \"loudness\": name the target in LUFS")
        ts = req.get("timestamps")                # speech marks: carried only when the request asks
        if ts is not None and ts is not False:
            if ts not in ("sentence", "phone"):
                raise ValueError(f"timestamps {ts!r}: False, \"sentence\" or \"phone\"")
            o["timestamps"] = ts
        return o

    @staticmethod
    def _format_kw(o: dict) -> dict:
        """the output-format keywords of audio_postprocess for resolved options: only the ones the request kept"""
        return {k: o[k] for k in ("sample_rate", "encoding", "loudness", "loudness_scope", "loudness_peak") if k in o}

    def _resolve_options(self, req: dict) -> dict:
        """_request_options(req) under the rules of the loaded model, what run() and run_batch work from: fragments, another
        speed and v3 / v4 parallel runs are never bucketed (reference TTS.py:1048-1062), and AP_BWE super-sampling applies to
        the v3 vocoder output only -- v1 / v2 / v2Pro / v4 ignore the key (TTS.py:1040, 1328, 1349).  A "lora_voice" that was
        not added raises ValueError here, before any GPU work, and so does a "best_of" that is no int in 1..16 or that comes
        with parallel_infer=False (check_best_of; the prompt-free case is refused as soon as the voice is known).  A
        "sample_rate" equal to the rate the request leaves at anyway (the model's, 48 kHz under super_sampling) and the
        encoding "pcm_s16" are dropped: such a request takes the default launches.  A rate the resampling kernel does not take
        from the model's raises ValueError here.  _output_sr() is asked only when the request names a rate."""
        o = self._request_options(req)
        check_best_of(o)
        if "lora_voice" in o:
            self._lora_voice(o["lora_voice"])
        if o["return_fragment"] or o["speed_factor"] != 1.0 or (self.configs.use_vocoder and o["parallel_infer"]):
            o["split_bucket"] = False
        o["super_sampling"] = o["super_sampling"] and self.configs.use_vocoder and self.configs.version == "v3"
        if o.get("encoding") == "pcm_s16":
            del o["encoding"]
        if "sample_rate" in o:
            from ..audio_io import output_rate_supported
            sr = self._output_sr()
            if o["super_sampling"]:
                self.init_sr_model()
                sr = self.sr_model.config["hr_sampling_rate"]
            if o["sample_rate"] == sr:
                del o["sample_rate"]
            elif not output_rate_supported(sr, o["sample_rate"]):
                raise ValueError(f"sample_rate {o['sample_rate']}: the resampling kernel does not take {sr} -> {o['sample_rate']} "
                                 "(its filter or its input window per tile is too large)")
        return o

    def plan_batch(self, plans: List[dict], mixed_sampling: bool = False, mixed_limits: bool = False) -> List[List[dict]]:
        """The AR launches of run_batch.  `plans[r]` = {"data": request r's to_batch batches, "no_prompt", "actual_seed",
        "opts"}.  Sentence j of batch bi of request r draws with the counter-RNG key (actual_seed_r + bi, j mod max_batch)
        -- the key it has in run(r) (the naive / prompt-free loop decodes every sentence alone: row 0).  Sentences are
        grouped by what is per launch (sampling parameters, parallel_infer, prompt-free, the decode budget run() gives them),
        sorted by length inside a group and cut into launches of at most max_batch rows.  Returns the launches: lists of
        {"r", "bi", "j", "len", "key", "group"}.  A request with "best_of" = n > 1 gives n entries per sentence, candidate c
        with "cand" = c and the key (seed, row + 1024 c): candidate 0 is the entry the request has without the key.
        mixed_sampling=True: the sampling parameters are per row (gsv_t2s_set_row_sampling) and no longer separate groups:
        their four slots of the group tuple hold None and every row carries "sampling" = (top_k, top_p, temperature,
        repetition_penalty) of its request.
        mixed_limits=True: the EOS horizon, the early stop and the step budget are per row (gsv_t2s_set_row_limits) and
        parallel_infer, prompt-free and the budget no longer separate groups: their three slots hold None and every row
        carries "limits" = (eos_mask_steps, early_stop_num, max_steps) -- (11 naive / prompt-free else 1, the configured early
        stop, the budget run() gives the sentence) -- and "no_prompt".  The keys are unchanged: naive rows keep row 0."""
        mb, max_seq = self.t2s_model.max_batch, self.t2s_model.max_seq
        groups: Dict[tuple, List[dict]] = {}
        for r, pl in enumerate(plans):
            o = pl["opts"]
            naive = pl["no_prompt"] or not o["parallel_infer"]
            P = 0 if pl["no_prompt"] else int(pl["P"])
            wanted = min(1500, int(early_stop_num(self.configs)) + 1)
            for bi, item in enumerate(pl["data"]):
                lens = [int(t.shape[-1]) for t in item["all_phones"]]
                for j, n in enumerate(lens):
                    # run() decodes this sentence in a launch of `lens` (naive: alone); the K/V arena bounds its budget there
                    need = (n if naive else max(lens[j - j % mb:j - j % mb + mb])) + P + 2
                    budget = min(wanted, max_seq - need)
                    sampling = (o["top_k"], o["top_p"], o["temperature"], o["repetition_penalty"])
                    per_launch = (bool(o["parallel_infer"]), bool(pl["no_prompt"]), budget)
                    g = ((None,) * 4 if mixed_sampling else sampling) + ((None,) * 3 if mixed_limits else per_launch)
                    e = dict(r=r, bi=bi, j=j, len=n + P, group=g, key=(pl["actual_seed"] + bi, 0 if naive else j % mb))
                    if mixed_sampling:
                        e["sampling"] = sampling
                    if mixed_limits:
                        e["limits"] = (11 if naive else 1, int(early_stop_num(self.configs)), budget)
                        e["no_prompt"] = bool(pl["no_prompt"])
                    if o.get("best_of", 1) > 1:
                        for c in range(o["best_of"]):
                            groups.setdefault(g, []).append(dict(e, cand=c, key=(e["key"][0], e["key"][1] + BEST_OF_ROW_STRIDE * c)))
                        continue
                    groups.setdefault(g, []).append(e)
        launches = []
        for g in groups:
            rows = sorted(groups[g], key=lambda e: e["len"])
            launches += [rows[i:i + mb] for i in range(0, len(rows), mb)]
        return launches

    sovits_max_frames = 25600     # frames (gaps included) of one shared SoVITS pass: the largest fold this engine has run

    @staticmethod
    def _voice_key(voice: dict, fields: Tuple[str, ...] = ("refer_spec", "sv_emb")) -> tuple:
        """what makes two requests' voices the same one for a shared stage: the stored objects the stage reads, themselves.
        The SoVITS pass reads the spectrogram list and the speaker embeddings; the flow-matching pass _CFM_VOICE_FIELDS."""
        return tuple(id(voice.get(f)) for f in fields)

    _CFM_VOICE_FIELDS = ("refer_spec", "prompt_semantic", "phones", "ref_mel", "raw_audio")   # what _prompt_features reads

    def plan_sovits(self, plans: List[dict]) -> List[List[Tuple[int, int]]]:
        """The waveform launches of run_batch(shared_sovits=True).  `plans[r]` = {"voice", "opts", "folds"}; folds[bi] is
        the number of kept semantic tokens of to_batch batch bi, which run() decodes as one time-folded sequence with seed
        actual_seed + bi.  A fold is one segment of SynthesizerTrn.decode_segments.  Shared: v1 / v2 / v2Pro / v2ProPlus
        folds at speed 1 with at least one token; the others are left to _synthesize_batch.  A launch holds at most
        VITS_MAX_VOICES distinct voices and at most sovits_max_frames frames, gaps included (n folds of T_s tokens take
        sum(2 T_s) + (n - 1) * segment_gap() frames); a fold larger than that gets a launch of its own.  Returns the
        launches, lists of (r, bi) in (r, bi) order."""
        from .. import _lib
        if getattr(self.configs, "use_vocoder", False):
            return []
        gap = self.vits_model.segment_gap()
        launches, cur, frames, voices = [], [], 0, set()
        for r, pl in enumerate(plans):
            if pl["opts"]["speed_factor"] != 1.0:
                continue
            key = self._voice_key(pl["voice"])
            for bi, tokens in enumerate(pl["folds"]):
                if tokens <= 0:
                    continue
                need = 2 * int(tokens)
                if cur and (frames + gap + need > self.sovits_max_frames or len(voices | {key}) > _lib.VITS_MAX_VOICES):
                    launches.append(cur)
                    cur, frames, voices = [], 0, set()
                frames += need + (gap if cur else 0)
                cur.append((r, bi))
                voices.add(key)
        if cur:
            launches.append(cur)
        return launches

    def plan_sovits_rows(self, plans: List[dict]) -> List[List[Tuple[int, int, int]]]:
        """The waveform launches of run_batch(shared_sovits=True, shared_speed=True).  `plans[r]` = {"voice", "opts",
        "folds", "sentences"}: folds as for plan_sovits, sentences[bi][k] the kept semantic tokens of sentence k of batch bi.
        A row is one segment of SynthesizerTrn.decode_segments(speeds=...): (r, bi, -1) is a whole speed-1 fold, as
        plan_sovits shares it; (r, bi, k), k >= 0, is sentence k of a request at another speed, which run() decodes on its
        own with speed_factor and seed actual_seed + bi.  Folds and sentences without tokens, and v3 / v4, are left out.
        A row of T tokens is 2T frames before the speed interpolation and F_s = int(2T / speed) + 1 after it and costs the
        larger; a launch holds at most sovits_max_frames frames, gaps included, and at most VITS_MAX_VOICES distinct
        voices; a row larger than that gets a launch of its own.  Returns the launches, lists of (r, bi, k) in that order."""
        from .. import _lib
        if getattr(self.configs, "use_vocoder", False):
            return []
        gap = self.vits_model.segment_gap()
        launches, cur, frames, voices = [], [], 0, set()
        for r, pl in enumerate(plans):
            speed = pl["opts"]["speed_factor"]
            key = self._voice_key(pl["voice"])
            for bi, tokens in enumerate(pl["folds"]):
                rows = [(-1, tokens)] if speed == 1.0 else list(enumerate(pl["sentences"][bi]))
                for k, t in rows:
                    if t <= 0:
                        continue
                    need = 2 * int(t) if speed == 1.0 else max(2 * int(t), int(2 * int(t) / speed) + 1)
                    if cur and (frames + gap + need > self.sovits_max_frames or len(voices | {key}) > _lib.VITS_MAX_VOICES):
                        launches.append(cur)
                        cur, frames, voices = [], 0, set()
                    frames += need + (gap if cur else 0)
                    cur.append((r, bi, k))
                    voices.add(key)
        if cur:
            launches.append(cur)
        return launches

    cfm_max_rows = 32             # rows (chunks of T_chunk frames) of one shared flow-matching pass: where the measured cost per
                                  # row stops falling, about 0.7 GB of workspace at T_chunk = 934

    def plan_cfm(self, plans: List[dict]) -> List[List[Tuple[int, int, int]]]:
        """The flow-matching passes of run_batch(shared_cfm=True).  `plans[r]` = {"opts", "T_min", "cfm_folds"}: T_min is the
        prompt length _prompt_features() gives request r's voice, cfm_folds[bi] the feature frames decode_encp makes of the
        sentences of to_batch batch bi (0 when nothing was generated).  Shared: v3 / v4 folds of parallel_infer requests with
        at least one frame, at any speed.  A fold is cut into rows as using_vocoder_synthesis_batched_infer cuts it
        (_chunk_cuts with the voice's chunk_len = T_chunk - T_min); every row is T_chunk frames whatever its voice.  Folds
        are grouped by sample_steps and guidance rate (every inference_cfg_rate <= 1e-5 is the one unguided group), and a
        group's rows fill passes of at most cfm_max_rows rows in (r, bi, k) order, so a fold may span two passes.  A guided
        row brings its unconditioned twin into the pass: a guided pass takes at most cfm_max_rows // 2 rows, so no pass runs
        the DiT over more than cfm_max_rows rows.  Returns the passes, lists of (r, bi, k)."""
        groups: Dict[Tuple[int, float], List[Tuple[int, int, int]]] = {}
        for row, steps, rate in TTS.plan_cfm_rows(self, plans):
            groups.setdefault((steps, rate), []).append(row)
        caps = {g: max(1, int(self.cfm_max_rows) // (2 if g[1] else 1)) for g in groups}
        return [rows[i:i + caps[g]] for g, rows in groups.items() for i in range(0, len(rows), caps[g])]

    def plan_cfm_rows(self, plans: List[dict]) -> List[Tuple[Tuple[int, int, int], int, float]]:
        """The rows of the shared flow-matching stage in (r, bi, k) order, as plan_cfm cuts them, each with its request's
        sample_steps and guidance rate (0.0 for every rate <= 1e-5): [((r, bi, k), sample_steps, rate)].  plan_cfm groups them
        into one-shot passes; run_batch(continuous_cfm=True) feeds them, in this order, to plan_cfm_session."""
        if not getattr(self.configs, "use_vocoder", False):
            return []
        vc = self.vocoder_configs
        out = []
        for r, pl in enumerate(plans):
            o = pl["opts"]
            if not o["parallel_infer"]:
                continue
            for bi, frames in enumerate(pl["cfm_folds"]):
                if frames <= 0:
                    continue
                n = len(self._chunk_cuts(int(frames), vc["T_chunk"] - int(pl["T_min"]), vc["overlapped_len"]))
                rate = o.get("inference_cfg_rate", 0)
                out.extend(((r, bi, k), int(o["sample_steps"]), float(rate) if cfg_guided(rate) else 0.0) for k in range(n))
        return out

    vocoder_max_frames = 32768    # mel frames of one shared vocoder pass.  No sweep of the cost per frame has been run yet
                                  # (DESIGN.md section 4h): this is the initial cap, which keeps every gapped layout far
                                  # below the engine's limit of 2^24 rows at the output rate for the v3 (x256) and v4 (x480)
                                  # vocoders (plan_vocoder checks the limit itself, gaps included)

    def plan_vocoder(self, plans: List[dict], gap: int = 0) -> List[List[Tuple[int, int]]]:
        """The vocoder passes of run_batch(shared_cfm=True, shared_vocoder=True).  `plans[r]` = {"opts", "T_min", "cfm_folds"}
        as plan_cfm takes them, after _shared_cfm_stage's flow-matching passes.  Shared: the folds plan_cfm shares (v3 / v4,
        parallel_infer, at least one frame).  A fold's mel is chunks * chunk_len frames, chunks as _chunk_cuts cuts it with
        its voice's chunk_len = T_chunk - T_min.  The folds fill passes in (r, bi) order; a pass ends before the fold that
        would take it past vocoder_max_frames frames, or past the engine's 2^24 output rows (`gap` = the vocoder's
        segment_gap() frames between neighbours), so a fold longer than the cap is a pass of its own.  Returns the passes,
        lists of (r, bi)."""
        if not getattr(self.configs, "use_vocoder", False):
            return []
        vc = self.vocoder_configs
        rows_cap = (1 << 24) // int(vc["upsample_rate"])     # gapped frames of a pass stay below this
        passes, cur, frames = [], [], 0
        for r, pl in enumerate(plans):
            if not pl["opts"]["parallel_infer"]:
                continue
            for bi, fold in enumerate(pl["cfm_folds"]):
                if fold <= 0:
                    continue
                chunk_len = vc["T_chunk"] - int(pl["T_min"])
                need = len(self._chunk_cuts(int(fold), chunk_len, vc["overlapped_len"])) * chunk_len
                if cur and (frames + need > int(self.vocoder_max_frames) or frames + need + len(cur) * gap >= rows_cap):
                    passes.append(cur)
                    cur, frames = [], 0
                cur.append((r, bi))
                frames += need
        if cur:
            passes.append(cur)
        return passes

    # ---- run_batch's stages: a plan is one request's dict, and a stage reads what the earlier ones wrote on it
    def _plan_request(self, req: dict, fragments: bool = False, timestamps: bool = False) -> dict:
        """Stage 1, per request, what run() does before its AR loop.  Reads the request and seeds the host generators (after
        the voice is resolved).  Writes the plan: `opts`, `voice`, `actual_seed`, `data` / `index` (to_batch), `no_prompt`,
        `P` (prompt tokens) and `frags`, one slot per to_batch batch for its sentences' waveforms, filled by later stages.
        fragments=True (gsv.serving only, which delivers a request fold by fold): a return_fragment request is planned too."""
        o = self._resolve_options(req)
        if o["return_fragment"] and not fragments:
            raise ValueError("run_batch returns whole utterances: return_fragment=True is not supported")
        if "timestamps" in o and not timestamps:      # timestamps=True: run_batch, which returns the marks
            raise ValueError("this caller returns (sr, audio): it does not pass timestamps=True, so it cannot return the marks")
        voice = self._request_voice(req)
        actual_seed = set_seed(o["seed"])
        segments = self._segments(req)
        no_prompt = voice["phones"] is None
        check_best_of(o, no_prompt)
        if no_prompt and self.configs.use_vocoder:
            raise NO_PROMPT_ERROR("v3/v4 need the prompt text (phones) of the reference audio")
        prompt_data = None if no_prompt else {"phones": voice["phones"], "bert_features": voice["bert_features"]}
        data, index = ([], []) if len(segments) == 0 else self.to_batch(
            segments, prompt_data=prompt_data, batch_size=o["batch_size"], threshold=o["batch_threshold"],
            split_bucket=o["split_bucket"], device=torch.device("cpu"), precision=self.precision)
        return dict(voice=voice, opts=o, actual_seed=actual_seed, data=data, index=index, no_prompt=no_prompt,
                    P=0 if no_prompt else int(voice["prompt_semantic"].numel()), frags=[None] * len(data),
                    **({"align": [[None] * len(item["phones"]) for item in data]} if o.get("timestamps") == "phone" else {}))

    @staticmethod
    def plan_sessions(launches: List[List[dict]]) -> List[Tuple[bool, List[dict]]]:
        """run_batch(continuous_ar=True): plan_batch's launches put back together by group.  Returns (session, rows) in
        plan_batch's order: the launches of a parallel-decode group with prompts become ONE queue for a decode session
        (Text2SemanticDecoder.infer_panel_continuous), rows in plan_batch's order with the keys and sampling tuples it gave
        them; prompt-free and naive groups stay the launches they are, unless plan_batch(mixed_limits=True) made the launches:
        their rows bring limits and all of them go through the session."""
        out: List[Tuple[bool, List[dict]]] = []
        for rows in launches:
            g = rows[0]["group"]
            session = g[4] is None or (g[4] and not g[5])   # mixed limits: every row; else parallel_infer and not prompt-free
            if session and out and out[-1][0] and out[-1][1][0]["group"] == g:
                out[-1][1].extend(rows)
            else:
                out.append((session, list(rows)))
        return out

    def _ar_stage(self, plans: List[dict], mixed_sampling: bool = False, continuous_ar: bool = False,
                  mixed_limits: bool = False) -> None:
        """Stage 2: every sentence of every request through the shared AR launches of plan_batch (mixed_sampling: launches
        shared across sampling parameters; a launch whose rows differ hands them over per row).  Reads `data`, `opts`,
        `voice`, `no_prompt`, `P`, `actual_seed`.  Writes run()'s pred_list / idx_list per batch: `preds[bi][j]`, the tokens
        of sentence j (prompt included), `idxs[bi][j]`, how many were generated (0 prompt-free), `kept[bi]` = _kept_tokens.
        continuous_ar: a group's launches are one decode session instead (plan_sessions).
        mixed_limits: launches shared across parallel_infer, prompt-free and budgets as well; a launch whose rows differ in
        them hands over limits and prompts per row (None for a prompt-free row), one that agrees takes the scalar path.
        A launch that holds candidate rows ("best_of") is decoded with log-probabilities; once every launch is back each such
        sentence keeps the tokens of the candidate choose_candidate picks, and `candidates[bi][j]` records the choice."""
        for pl in plans:
            pl["preds"] = [[None] * len(item["all_phones"]) for item in pl["data"]]
            pl["idxs"] = [[None] * len(item["all_phones"]) for item in pl["data"]]
        cands: Dict[tuple, Dict[int, tuple]] = {}       # (r, bi, j) -> candidate -> (its dict, y)
        pkw = dict(mixed_sampling=True) if mixed_sampling else {}
        if mixed_limits:
            pkw["mixed_limits"] = True
        launches = self.plan_batch(plans, **pkw)
        work = self.plan_sessions(launches) if continuous_ar else [(False, rows) for rows in launches]
        for session, rows in work:
            o = plans[rows[0]["r"]]["opts"]
            kw = {}
            if mixed_sampling and len({e["sampling"] for e in rows}) > 1:     # a uniform launch takes the scalar path
                kw["row_sampling"] = [e["sampling"] for e in rows]
            if mixed_limits:
                lims, free = [e["limits"] for e in rows], [e["no_prompt"] for e in rows]
                uniform = len(set(lims)) == 1 and len(set(free)) == 1
                no_prompt, eos_steps, steps = uniform and free[0], lims[0][0], max(l_[2] for l_ in lims)
                if not uniform or (session and (no_prompt or eos_steps != 1)):
                    kw["row_limits"] = lims
            else:
                no_prompt = rows[0]["group"][5]
                free = [no_prompt] * len(rows)
                eos_steps, steps = 11 if no_prompt or not o["parallel_infer"] else 1, rows[0]["group"][6]
            want_lp = any("cand" in e for e in rows)
            if want_lp:
                kw["logprobs"] = True
            items = [plans[e["r"]]["data"][e["bi"]] for e in rows]
            x = [it["all_phones"][e["j"]] for it, e in zip(items, rows)]
            bert = [it["all_bert_features"][e["j"]] for it, e in zip(items, rows)]
            prompts = None if no_prompt and "row_limits" not in kw else \
                [None if f else plans[e["r"]]["voice"]["prompt_semantic"].view(-1) for e, f in zip(rows, free)]
            if session:
                y, idx = self.t2s_model.infer_panel_continuous(
                    x, prompts, bert, o["top_k"], o["top_p"], early_stop_num(self.configs), o["temperature"],
                    o["repetition_penalty"], rng_keys=[e["key"] for e in rows], max_steps=steps, **kw)
            else:
                y, idx = self.t2s_model._run(x, prompts, bert, o["top_k"], o["top_p"], early_stop_num(self.configs), o["temperature"],
                                             o["repetition_penalty"], eos_mask_steps=eos_steps,
                                             max_steps=steps, rng_keys=[e["key"] for e in rows], **kw)
            for k, (e, y_, i_, f) in enumerate(zip(rows, y, idx, free)):
                if "cand" in e:
                    c = dict(tokens=y_[-i_:] if i_ > 0 else y_[:0], logprobs=self.t2s_model.last_logprobs[k].cpu().numpy(), n=i_,
                             cut=self.t2s_model.last_cut[k])
                    cands.setdefault((e["r"], e["bi"], e["j"]), {})[e["cand"]] = (c, y_)
                    continue
                plans[e["r"]]["preds"][e["bi"]][e["j"]] = y_
                plans[e["r"]]["idxs"][e["bi"]][e["j"]] = 0 if f else i_
        for (r, bi, j), by_c in sorted(cands.items()):
            pl = plans[r]
            k, rec = choose_candidate(pl["opts"], [by_c[c][0] for c in sorted(by_c)])
            pl["preds"][bi][j], pl["idxs"][bi][j] = by_c[k][1], by_c[k][0]["n"]
            pl.setdefault("candidates", [[None] * len(item["all_phones"]) for item in pl["data"]])[bi][j] = rec
        for pl in plans:
            pl["kept"] = [self._kept_tokens(p, i, pl["no_prompt"]) for p, i in zip(pl["preds"], pl["idxs"])]
        self._wait_stream()

    def _shared_sovits_stage(self, plans: List[dict], shared_speed: bool = False,
                             folds: Optional[Iterable[Tuple[int, int]]] = None) -> None:
        """shared_sovits, v1 / v2 / v2Pro: every fold (request r, to_batch batch bi) that plan_sovits shares is one segment,
        with r's voice, of a SynthesizerTrn.decode_segments pass; with shared_speed, so is every sentence of a request at
        another speed that plan_sovits_rows shares, at that speed.  Reads `kept`, `voice`, `opts`, `actual_seed`, `data`.
        Writes `folds` and `sentences` (kept tokens per batch / per sentence, the planners' inputs), `frags[bi]` of every
        shared fold and `frags[bi][k]` of every shared sentence (None where a sentence was left out).
        `folds` (gsv.serving, which delivers a streaming request fold by fold): only these (r, bi) are planned and decoded;
        `kept[bi]` of the others is not read (it may still be None)."""
        up = math.prod(self.vits_model.upsample_rates)
        only = None if folds is None else set(folds)
        for r, pl in enumerate(plans):
            pl["sentences"] = [[int(p_.shape[0]) for p_ in pl["kept"][bi][0]] if only is None or (r, bi) in only else []
                               for bi in range(len(pl["kept"]))]
            pl["folds"] = [sum(t) for t in pl["sentences"]]
        dev_voice: Dict[tuple, tuple] = {}          # one device refer list per distinct voice: one voice slot
        launches = self.plan_sovits_rows(plans) if shared_speed else [[(r, bi, -1) for r, bi in launch]
                                                                      for launch in self.plan_sovits(plans)]
        for launch in launches:
            codes, phones, voices, seeds, speeds, cuts, align = [], [], [], [], [], [], []
            for r, bi, k in launch:
                pl = plans[r]
                pred = pl["kept"][bi][0]
                keep = [k] if k >= 0 else [j for j, p_ in enumerate(pred) if p_.shape[0] > 0]
                spans, c0, p0 = [], 0, 0        # "timestamps": "phone": one alignment span per sentence of the segment
                for j in keep if "align" in pl else []:
                    spans.append((c0, int(pred[j].shape[0]), p0, int(pl["data"][bi]["phones"][j].shape[0]), j))
                    c0, p0 = c0 + spans[-1][1], p0 + spans[-1][3]
                align.append(spans)
                codes.append(torch.cat([pred[j] for j in keep]).view(1, 1, -1))
                phones.append(torch.cat([pl["data"][bi]["phones"][j] for j in keep]).view(1, -1))
                vk = self._voice_key(pl["voice"])
                if vk not in dev_voice:
                    refer, sv_kw = self._voice_refer(pl["voice"])
                    dev_voice[vk] = (refer, sv_kw.get("sv_emb"))
                voices.append(dev_voice[vk])
                seeds.append(pl["actual_seed"] + bi)
                speeds.append(pl["opts"]["speed_factor"] if k >= 0 else 1.0)
                cuts.append([int(p_.shape[0]) * 2 * up for p_ in pred])
            speed_kw = {} if all(v == 1.0 for v in speeds) else dict(speeds=speeds)
            marked = any(align)
            wavs = self.vits_model.decode_segments(codes, phones, voices, seeds, **speed_kw,
                                                   **({"align": [[sp[:4] for sp in a] for a in align]} if marked else {}))
            got = iter(self.vits_model.last_alignment if marked else [])
            for (r, bi, k), a in zip(launch, align):
                for c0, nc, p0, nph, j in a:
                    plans[r]["align"][bi][j] = (2 * nc,) + next(got)
            for (r, bi, k), wav, cut in zip(launch, wavs, cuts):
                if k < 0:
                    plans[r]["frags"][bi] = list(torch.split(wav[0, 0], cut))
                else:
                    if plans[r]["frags"][bi] is None:
                        plans[r]["frags"][bi] = [None] * len(cut)
                    plans[r]["frags"][bi][k] = wav[0, 0]
        self.vits_model.invalidate_refer()          # the engine's cached reference terms are the last slot's voice

    def _continuous_cfm_passes(self, plans: List[dict], fold_in: dict, prompts: dict, voice_of: list) -> Dict[Tuple[int, int], list]:
        """continuous_cfm: the rows of every (sample_steps, guidance rate) group through ONE flow-matching session
        (CFM.open_session) on the schedule of plan_cfm_session: FIFO admission into at most cfm_max_rows DiT rows, every step()
        call runs until the next row finishes, and a finished row's slot goes to the next waiting row.  The session's cap is
        cfm_max_rows clipped to the engine's 64 DiT rows per session, and at least 2 when a row is guided.  Each row carries the
        prompt, seed, adapter, step count and rate it carries in the one-shot passes.  -> fold_out as _shared_cfm_stage builds it."""
        rows = self.plan_cfm_rows(plans)
        fold_out: Dict[Tuple[int, int], list] = {}
        if not rows:
            return fold_out
        # a session has at most CFM_SESSION_MAX_ROWS (64) DiT rows: a larger cfm_max_rows is clipped to it (the grouped passes
        # have no such limit).  cfm_max_rows = 1 still serves a guided row, as plan_cfm does (a pass of one row and its twin)
        cap = min(int(self.cfm_max_rows), CFM_SESSION_MAX_ROWS)
        cap = max(cap, 2 if any(rate > 0.0 for _, _, rate in rows) else 1)
        schedule = plan_cfm_session([(steps, rate > 0.0) for _, steps, rate in rows], cap)
        got: Dict[Tuple[int, int], dict] = {}
        T_chunk = int(fold_in[rows[0][0][:2]][0].shape[1])
        with self.vits_model.cfm.open_session(cap, T_chunk) as sess:
            in_slot: Dict[int, int] = {}
            for admit, k in schedule:
                if admit:
                    at = [rows[i][0] for i in admit]
                    mu = torch.cat([fold_in[(r, bi)][0][kk:kk + 1] for r, bi, kk in at], 0)
                    mels = [prompts[voice_of[r]][3] for r, _, _ in at]
                    seeds = [CFM.row_seed(plans[r]["actual_seed"] + bi, kk) for r, bi, kk in at]
                    names = [plans[r]["opts"].get("lora_voice") for r, _, _ in at]
                    lora_kw = dict(adapters=[None if n is None else self._lora_voice(n)[1] for n in names]) if any(names) else {}
                    slots = sess.admit(mu, mels, [rows[i][1] for i in admit], [rows[i][2] for i in admit], seeds=seeds, **lora_kw)
                    in_slot.update(zip(slots, admit))
                for slot in sess.step(k):
                    (r, bi, kk), _, _ = rows[in_slot.pop(slot)]
                    Tp = int(prompts[voice_of[r]][3].shape[2])
                    dt = fold_in[(r, bi)][0].dtype           # what CFM.inference_rows returns for this mu
                    pred = sess.fetch(slot).to(dt if dt in (torch.float16, torch.float32) else torch.float32)
                    got.setdefault((r, bi), {})[kk] = pred[None, :, Tp:]
            assert not in_slot, "plan_cfm_session left rows in the session"
        for key in sorted(got):
            fold_out[key] = [got[key][kk] for kk in sorted(got[key])]
        return fold_out

    def _shared_cfm_stage(self, plans: List[dict], shared_vocoder: bool = False, continuous_cfm: bool = False,
                          folds: Optional[Iterable[Tuple[int, int]]] = None) -> None:
        """shared_cfm, v3 / v4: every chunk of every fold that plan_cfm shares is one row, with its voice's prompt mel, the
        noise key run() gives it and its request's LoRA adapter (the key "lora_voice"), of a CFM.inference_rows pass; vocoder and SOLA stay per fold, unless shared_vocoder: then
        the folds' mels go through the plan_vocoder passes of the vocoder's forward_segments, and only SOLA and the cuts stay
        per fold.  Reads `preds`, `kept`, `voice`, `opts`, `actual_seed`, `data`.  Writes `cfm_folds` (feature frames per
        batch) and `T_min` (the voice's prompt length), plan_cfm's inputs, and `frags[bi]` of every shared fold.
        `folds` (gsv.serving): only these (r, bi) go through the stage, as for _shared_sovits_stage."""
        prompts, fold_in, voice_of = self._cfm_encode(plans, **({} if folds is None else {"folds": folds}))
        if continuous_cfm:
            fold_out = self._continuous_cfm_passes(plans, fold_in, prompts, voice_of)
        else:
            fold_out = self._grouped_cfm_passes(plans, fold_in, prompts, voice_of)
        self._vocode_folds(plans, fold_in, fold_out, shared_vocoder)

    def _cfm_encode(self, plans: List[dict], prompts: Optional[Dict[tuple, tuple]] = None,
                    folds: Optional[Iterable[Tuple[int, int]]] = None) -> Tuple[dict, dict, list]:
        """The first half of the shared flow-matching stage, up to the rows the DiT takes: per distinct voice (and LoRA
        encoder) one _prompt_features(), per fold with generated tokens one _fold_chunks().  Reads `kept`, `preds`, `voice`,
        `opts`, `data`; writes `cfm_folds` and `T_min`.  `prompts`: a cache of _prompt_features() by voice key that the
        caller keeps between calls (gsv.serving encodes request by request); entries are added to it.  `folds`: only these
        (r, bi) are encoded, the others count as folds without frames and their `kept[bi]` is not read.
        -> (prompts, fold_in[(r, bi)] = (rows [chunks, T_chunk, 512], lens, pad_len), voice_of[r] = r's key in prompts)"""
        prompts = {} if prompts is None else prompts            # _prompt_features() per distinct voice
        fold_in: Dict[Tuple[int, int], tuple] = {}  # (rows [chunks, T_chunk, 512], lens, pad_len)
        voice_of: List[Optional[tuple]] = [None] * len(plans)
        only = None if folds is None else set(folds)
        for r, pl in enumerate(plans):
            pl["cfm_folds"], pl["T_min"] = [0] * len(pl["data"]), 0
            if not pl["opts"]["parallel_infer"] or not pl["data"]:
                continue
            lora = pl["opts"].get("lora_voice")
            with self._with_prompt_cache(dict(pl["voice"])):
                # a LoRA voice with an encoder-side engine of its own has its own prompt features of the same reference audio
                vk = voice_of[r] = self._voice_key(pl["voice"], self._CFM_VOICE_FIELDS)
                if lora is not None:
                    vk = voice_of[r] = vk + (id(self._lora_voice(lora)[0]),)
                if vk not in prompts:
                    prompts[vk] = self._prompt_features(*([] if lora is None else [lora]))
                prompt = prompts[vk]
                pl["T_min"] = prompt[4]
                for bi, item in enumerate(pl["data"]):
                    if only is not None and (r, bi) not in only:
                        continue
                    idx_list = pl["kept"][bi][1]
                    if sum(int(i) for i in idx_list) <= 0:
                        continue
                    al = [] if "align" in pl else None       # "timestamps": "phone": decode_encp aligns each sentence (4w)
                    fold_in[(r, bi)] = self._fold_chunks(prompt, idx_list, pl["preds"][bi],
                                                         [ph.to(self.configs.device) for ph in item["phones"]],
                                                         pl["opts"]["speed_factor"], *([] if lora is None else [lora]),
                                                         **({} if al is None else {"align_out": al}))
                    if al is not None:
                        pl["align"][bi] = al
                    pl["cfm_folds"][bi] = sum(fold_in[(r, bi)][1])
        return prompts, fold_in, voice_of

    def _grouped_cfm_passes(self, plans: List[dict], fold_in: dict, prompts: dict, voice_of: list) -> Dict[Tuple[int, int], list]:
        """the one-shot passes of plan_cfm: one CFM.inference_rows call per pass -> fold_out[(r, bi)] = the fold's rows in order"""
        fold_out: Dict[Tuple[int, int], list] = {}
        for rows in self.plan_cfm(plans):
            mu = torch.cat([fold_in[(r, bi)][0][k:k + 1] for r, bi, k in rows], 0)
            mels = [prompts[voice_of[r]][3] for r, _, _ in rows]
            seeds = [CFM.row_seed(plans[r]["actual_seed"] + bi, k) for r, bi, k in rows]
            o = plans[rows[0][0]]["opts"]           # a pass is of one (sample_steps, guidance rate) group
            names = [plans[r]["opts"].get("lora_voice") for r, _, _ in rows]            # rows of any voice share the pass
            lora_kw = dict(adapters=[None if n is None else self._lora_voice(n)[1] for n in names]) if any(names) else {}
            pred = self.vits_model.cfm.inference_rows(mu, mels, o["sample_steps"], seeds=seeds,
                                                      inference_cfg_rate=o["inference_cfg_rate"], **lora_kw)
            for n, (r, bi, k) in enumerate(rows):
                fold_out.setdefault((r, bi), []).append(pred[n:n + 1, :, mels[n].shape[2]:])
        return fold_out

    def _vocode_folds(self, plans: List[dict], fold_in: dict, fold_out: dict, shared_vocoder: bool) -> None:
        """the folds' mels (fold_out) -> `frags[bi]`: one vocoder call per fold, or the plan_vocoder passes of forward_segments"""
        for (r, bi), got in fold_out.items():        # a fold is finished when all its rows are back
            assert len(got) == fold_in[(r, bi)][0].shape[0]
        if not shared_vocoder:
            for (r, bi), got in fold_out.items():
                _, lens, pad_len = fold_in[(r, bi)]
                plans[r]["frags"][bi] = self._fold_audio(torch.cat(got, 0), lens, pad_len)
            return
        for folds in self.plan_vocoder(plans, gap=self.vocoder.segment_gap()):
            audios = self.vocoder.forward_segments([self._fold_mel(torch.cat(fold_out[f], 0)) for f in folds])
            for (r, bi), audio in zip(folds, audios):
                _, lens, pad_len = fold_in[(r, bi)]
                plans[r]["frags"][bi] = self._fold_tail(audio[0][0], int(fold_out[(r, bi)][0].shape[2]), lens, pad_len)

    def _finish_request(self, pl: dict, sr: int) -> Tuple[int, np.ndarray]:
        """Last stage, per request, with its voice as the prompt cache: the batches no shared stage took go through
        _synthesize_batch as in run(), then audio_postprocess.  Reads `frags`, `preds`, `kept`, `voice`, `opts`,
        `actual_seed`, `data`, `index`; fills the rest of `frags`; returns the request's (sr, int16 audio)."""
        if not pl["data"]:
            return silence()
        o = pl["opts"]
        with self._with_prompt_cache(dict(pl["voice"])) as voice:
            voice_refer = self._voice_refer(voice)
            for bi, item in enumerate(pl["data"]):
                if pl["frags"][bi] is None or any(f is None for f in pl["frags"][bi]):
                    self._synthesize_fold(pl, bi, voice_refer)
            self._wait_stream()
            result = self.audio_postprocess(pl["frags"], sr, pl["index"], o["speed_factor"], o["split_bucket"],
                                            o["fragment_interval"], o["super_sampling"], **self._format_kw(o))
            if "timestamps" not in o:
                return result
            # speech marks, as run() builds them
            sents = [s for bi in range(len(pl["data"])) for s in self._fold_sentences(pl, bi)]
            order = sorted(range(len(sents)), key=lambda i: sents[i]["index"]) if o["split_bucket"] else None
            marks = build_marks(sents, sr, int(self.configs.sampling_rate * o["fragment_interval"]), order=order)
            return result + (marks,)

    @staticmethod
    def _fold_sentences(pl: dict, bi: int) -> List[dict]:
        """build_marks' input for the sentences of fold `bi` of a planned request whose waveforms exist (`frags[bi]`): index,
        text, samples and, with "timestamps": "phone", the alignment its waveform pass left in `align[bi]`"""
        item, sents = pl["data"][bi], []
        for k, f in enumerate(pl["frags"][bi]):
            s = dict(index=pl["index"][bi][k], text=item["norm_text"][k], n_samples=int(f.shape[0]))
            if "align" in pl:
                a = pl["align"][bi][k]
                if a is None:               # a sentence without tokens inside a shared fold: no frames, every phoneme empty
                    a = (0, np.zeros(int(item["phones"][k].shape[0]), np.int32), float("-inf"))
                s.update(phones=item["phones"][k].tolist(), nf=a[0], ends=a[1], score=a[2])
            w2p = pl["data"][bi].get("word2ph")
            if w2p is not None and w2p[k] is not None:
                s["word2ph"] = w2p[k]
            sents.append(s)
        return sents

    def _synthesize_fold(self, pl: dict, bi: int, voice_refer) -> None:
        """`frags[bi]` of a planned request through _synthesize_batch where a shared stage left the fold or some of its sentences
        out, with the alignment of what it decodes merged into `align[bi]` (the shared pass holds the rest)"""
        pred, idx_list = pl["kept"][bi]
        al = [] if "align" in pl else None
        pl["frags"][bi] = self._synthesize_batch(pl["data"][bi], pred, pl["preds"][bi], idx_list, bi, pl["actual_seed"], pl["opts"],
                                                 voice_refer, have=pl["frags"][bi], **({} if al is None else {"align_out": al}))
        if al is not None:
            pl["align"][bi] = [a if a is not None else b for a, b in zip(al, pl["align"][bi])]

    def _output_sr(self) -> int:
        """the rate of the waveform stage: the SoVITS model's, v3 / v4 the vocoder's (which must be loaded)"""
        if self.configs.use_vocoder and self.vocoder is None:
            raise RuntimeError("init_vocoder() first")
        return self.vocoder_configs["sr"] if self.configs.use_vocoder else self.configs.sampling_rate

    def _wait_stream(self) -> None:
        # stream-level wait only: the engine calls before it already synchronised their own streams, and a DEVICE-wide
        # synchronize intermittently stalls 20-30 ms on this ROCm build
        torch.cuda.current_stream(self.configs.device).synchronize()

    @torch.no_grad()
    def run_batch(self, requests: List[dict], shared_sovits: bool = False, shared_cfm: bool = False,
                  shared_speed: bool = False, mixed_sampling: bool = False,
                  shared_vocoder: bool = False, shared_bert: bool = False,
                  shared_hubert: bool = False, shared_sv: bool = False,
                  device_frontend: bool = False, continuous_ar: bool = False,
                  continuous_cfm: bool = False, mixed_limits: bool = False) -> List[Tuple[int, np.ndarray]]:
        """Several requests, each with its own reference voice, through shared AR decodes.  Each request dict takes the
        keys run() accepts plus an optional "voice" (make_voice); without one it uses its ref_audio_path / prompt_text
        (through make_voice's LRU) or the current prompt cache.  Returns one (sr, int16 audio) per request, in order: what
        run(request) alone returns.  self.prompt_cache is not changed.  return_fragment is not supported.
        shared_sovits=True: v1 / v2 / v2Pro / v2ProPlus requests at speed 1 take their waveforms from shared segmented passes
        over all voices (_shared_sovits_stage) instead of one decode per to_batch batch.  shared_cfm=True: v3 / v4
        parallel_infer requests take their flow-matching stage from shared passes over all voices' chunks (_shared_cfm_stage).
        shared_speed=True (with shared_sovits=True): the sentences of v1 / v2 / v2Pro / v2ProPlus requests at speed_factor != 1
        join the same segmented passes, each at its own speed, instead of one decode per sentence.
        mixed_sampling=True: requests with different top_k / top_p / temperature / repetition_penalty share AR launches, each
        row sampling with its own request's values (plan_batch(mixed_sampling=True)); every request still gets the tokens it
        gets without the keyword.
        shared_vocoder=True (with shared_cfm=True; ValueError without it on a v3 / v4 model): the folds of the shared
        flow-matching stage are vocoded in shared segmented passes over all voices (plan_vocoder, the vocoder's
        forward_segments) instead of one vocoder call per fold.
        shared_bert=True: the raw texts of all requests go through one TextPreprocessor.preprocess_many before stage 1, so the
        zh BERT features of every sentence of every request come from one packed pass (requests that bring `segments`, and all
        requests under a `text_frontend`, are left as they are).
        shared_hubert=True: the requests that name a `ref_audio_path` and bring no `voice` get their voices from one make_voices
        call before planning: one packed HuBERT pass over the reference audios the voice LRU does not hold, instead of one
        pass per voice.
        shared_sv=True (implies the make_voices route of shared_hubert): on a v2Pro / v2ProPlus model those voices also take their
        speaker embeddings, main and auxiliary, from one packed ERes2NetV2 pass (make_voices(shared_sv=True)).
        device_frontend=True (with shared_hubert or shared_sv, else ValueError): that make_voices call reads the reference files on
        the host and resamples, normalises and frames them on the device (make_voices(device_frontend=True)).
        continuous_ar=True: each group of plan_batch (parallel decode with prompts) is decoded through one decode session
        (plan_sessions, Text2SemanticDecoder.infer_panel_continuous) instead of launches of max_batch rows: a sentence that
        ends early hands its slot to the next one.  Same keys, same sampling values, the same tokens per sentence.
        continuous_cfm=True (with shared_cfm=True, else ValueError): the shared flow-matching stage runs through one session
        (CFM.open_session) on the schedule of plan_cfm_session instead of one pass per (sample_steps, guidance rate) group:
        requests with different settings share the DiT launches, each row with its own step count and rate, and a finished
        row's place goes to the next waiting row.  Seeds, prompts, LoRA adapters, the vocoder and SOLA are those of shared_cfm.
        mixed_limits=True: naive (parallel_infer=False), prompt-free and arena-bound sentences share AR launches (or, with
        continuous_ar=True, the decode session) with the others: each row brings its EOS horizon, early stop and step budget
        (plan_batch(mixed_limits=True), gsv_t2s_set_row_limits) and every request still gets the tokens it gets without the
        keyword.
        A request with "best_of" = n > 1 decodes n candidates per sentence as further rows of the shared launches and keeps
        one (plan_batch, select_candidate; "best_of_score": a callable in its place); last_candidates[r][bi][j] then lists
        dict(n, mean_logprob, cut, chosen) per candidate, and is [] for a request without the key.
        No keyword changes anything for the other model family."""
        if self.t2s_model is None or self.vits_model is None:
            raise RuntimeError("init_t2s_weights / init_vits_weights first")
        if shared_vocoder and self.configs.use_vocoder and not shared_cfm:
            raise ValueError("shared_vocoder=True vocodes the folds of the shared flow-matching stage: pass shared_cfm=True too")
        if continuous_cfm and not shared_cfm:
            raise ValueError("continuous_cfm=True runs the shared flow-matching stage through a session: pass shared_cfm=True too")
        if device_frontend and not (shared_hubert or shared_sv):
            raise ValueError("device_frontend=True is the front-end of the shared make_voices call: pass shared_hubert=True or shared_sv=True too")
        self.stop_flag = False
        if shared_bert:
            requests = self._with_shared_segments(requests)
        if shared_hubert or shared_sv:
            requests = self._with_shared_voices(requests, shared_sv=shared_sv, device_frontend=device_frontend)
        # the keyword goes along only with a request that brings the key: a stage that predates it (a subclass, a stub) keeps working
        plans = [self._plan_request(req, **({} if req.get("timestamps") in (None, False) else {"timestamps": True}))
                 for req in requests]
        self._ar_stage(plans, mixed_sampling=mixed_sampling, **({"continuous_ar": True} if continuous_ar else {}),
                       **({"mixed_limits": True} if mixed_limits else {}))
        self.last_candidates = [pl.get("candidates", []) for pl in plans]
        self.last_loudness = []
        sr = self._output_sr()
        if shared_sovits and not self.configs.use_vocoder:
            self._shared_sovits_stage(plans, shared_speed=shared_speed)
        if shared_cfm and self.configs.use_vocoder:
            # the keyword goes along only when it is set: a stage that predates it (a subclass, a stub) keeps working without it
            self._shared_cfm_stage(plans, shared_vocoder=shared_vocoder, **({"continuous_cfm": True} if continuous_cfm else {}))
        results, reports = [], []
        for pl in plans:                                 # the reports of the requests with "loudness", in request order
            self.last_loudness = []
            results.append(self._finish_request(pl, sr))
            reports += self.last_loudness
        self.last_loudness = reports
        self.last_timestamps = [res[2] if isinstance(res, tuple) and len(res) == 3 else [] for res in results]      # per request, [] without the key
        return results

    def serve(self, **scheduler_kw):
        """Requests as they arrive instead of a closed list: a started `gsv.serving.Server` over a `Scheduler` of this
        pipeline (keywords: slots, chunk, admit_min, wave_hold, the shared_* flags, and on v3 / v4 continuous_cfm, cfm_rows,
        cfm_chunk: the waveform stage as an open flow-matching session).  `submit(request)` returns a Future of
        what run_batch([request]) returns; until `shutdown()` the server's loop thread owns the pipeline."""
        from ..serving import Scheduler, Server
        return Server(Scheduler(self, **scheduler_kw))

    # ---- the pipeline (reference TTS.py:984-1365) ---------------------------------------------
    @torch.no_grad()
    def run(self, inputs: dict) -> Generator[Tuple[int, np.ndarray], None, None]:
        self.stop_flag = False
        o = self._resolve_options(inputs)
        actual_seed = set_seed(o["seed"])
        try:
            if self.t2s_model is None or self.vits_model is None:
                raise RuntimeError("init_t2s_weights / init_vits_weights first")
            # ---- reference audio and prompt text (reference TTS.py:1078-1120)
            self._prepare_prompt(inputs)
            t0 = time.perf_counter()
            segments = self._segments(inputs)
            if len(segments) == 0:
                yield silence()
                return
            pc = self.prompt_cache
            prompt_data = None if pc["phones"] is None else {"phones": pc["phones"], "bert_features": pc["bert_features"]}
            check_best_of(o, prompt_data is None)
            self.last_candidates = [[]] if "best_of" in o else []
            self.last_loudness, loud_reports = [], []
            ts, sents, ts_offset = o.get("timestamps"), [], 0.0          # speech marks
            self.last_timestamps = []
            ts_gap = int(self.configs.sampling_rate * o["fragment_interval"])      # audio_postprocess's
            t1 = time.perf_counter()
            # token ids stay on the host here: the engines pack a whole batch and move it with ONE copy
            # (the reference's per-item .to(device), TTS.py:899-912, is ~75 tiny transfers per batch of 32)
            data, batch_index_list = self.to_batch(segments, prompt_data=prompt_data, batch_size=o["batch_size"],
                                                   threshold=o["batch_threshold"], split_bucket=o["split_bucket"],
                                                   device=torch.device("cpu"), precision=self.precision)
            t2 = time.perf_counter()
            infer = self.t2s_model.infer_panel_batch_infer if o["parallel_infer"] else self.t2s_model.infer_panel_naive_batched
            voice_refer = self._voice_refer(self.prompt_cache)
            audio, t_34, t_45 = [], 0.0, 0.0
            sr = self._output_sr()
            self.last_generated_tokens = 0
            for bi, item in enumerate(data):
                t3 = time.perf_counter()
                # no prompt text (reference TTS.py:1124-1131, 1223-1226): nothing is prepended and the AR decoder runs
                # prompt-free through the naive loop; v3/v4 require a prompt (TTS.py:1062-1063)
                no_prompt = prompt_data is None
                if no_prompt and self.configs.use_vocoder:
                    raise NO_PROMPT_ERROR("v3/v4 need the prompt text (phones) of the reference audio")
                prompt = None if no_prompt else self.prompt_cache["prompt_semantic"].view(1, -1).expand(len(item["all_phones"]), -1)
                if "best_of" in o:
                    pred_list, idx_list, rec = self._decode_best_of(item, prompt, o, actual_seed + bi)
                    self.last_candidates[0].append(rec)
                else:
                    pred_list, idx_list = infer(item["all_phones"], item["all_phones_len"], prompt,
                                                item["all_bert_features"], top_k=o["top_k"], top_p=o["top_p"],
                                                temperature=o["temperature"], early_stop_num=early_stop_num(self.configs),
                                                max_len=item["max_len"], repetition_penalty=o["repetition_penalty"],
                                                seed=actual_seed + bi)
                self._wait_stream()
                t4 = time.perf_counter()
                t_34 += t4 - t3
                pred, idx_list = self._kept_tokens(pred_list, idx_list, no_prompt)
                self.last_generated_tokens += int(sum(idx_list))
                al = [] if ts == "phone" else None
                frags = self._synthesize_batch(item, pred, pred_list, idx_list, bi, actual_seed, o, voice_refer,
                                               **({} if al is None else {"align_out": al}))
                if ts:
                    fold = [dict(index=batch_index_list[bi][k], text=item["norm_text"][k], n_samples=int(f.shape[0]),
                                 **({} if al is None else dict(phones=item["phones"][k].tolist(), nf=al[k][0], ends=al[k][1],
                                                               score=al[k][2])),
                                 **({} if item.get("word2ph") is None or item["word2ph"][k] is None
                                    else {"word2ph": item["word2ph"][k]})) for k, f in enumerate(frags)]
                self._wait_stream()
                t5 = time.perf_counter()
                t_45 += t5 - t4
                if o["return_fragment"]:
                    frag = self.audio_postprocess([frags], sr, None, o["speed_factor"], False, o["fragment_interval"],
                                                  o["super_sampling"], **self._format_kw(o))
                    if "loudness" in o:                                 # one report list per fragment, gathered over the run
                        loud_reports += self.last_loudness
                        self.last_loudness = loud_reports
                    if ts:        # times relative to the fragment, and where the fragment starts in the request's stream
                        marks = [dict(m, offset=ts_offset) for m in build_marks(fold, sr, ts_gap)]
                        ts_offset += sum(s["n_samples"] + ts_gap for s in fold) / sr
                        self.last_timestamps = marks
                        frag = frag + (marks,)
                    yield frag
                else:
                    audio.append(frags)
                    if ts:
                        sents += fold
                if self.stop_flag:
                    yield silence()
                    return
            self.last_timing = (t1 - t0, t2 - t1, t_34, t_45)
            if not o["return_fragment"]:
                if len(audio) == 0:
                    yield silence()
                    return
                t6 = time.perf_counter()
                result = self.audio_postprocess(audio, sr, batch_index_list, o["speed_factor"], o["split_bucket"],
                                                o["fragment_interval"], o["super_sampling"], **self._format_kw(o))
                self.last_postprocess_s = time.perf_counter() - t6
                if ts:            # output order: submission order when the buckets are put back, else batch order
                    order = sorted(range(len(sents)), key=lambda i: sents[i]["index"]) if o["split_bucket"] else None
                    self.last_timestamps = build_marks(sents, sr, ts_gap, order=order)
                    result = result + (self.last_timestamps,)
                yield result
        except Exception as e:
            traceback.print_exc()
            # the reference yields 1 s of silence, rebuilds both models, then re-raises (TTS.py:1352-1363)
            yield silence()
            try:
                if self._t2s_state is not None and self._vits_state is not None:
                    self.t2s_model = None
                    self.vits_model = None
                    lora_voices = self._lora_voices
                    self.init_t2s_weights(self.configs.t2s_weights_path, state=self._t2s_state)
                    self.init_vits_weights(self.configs.vits_weights_path, state=self._vits_state)
                    for name, v in lora_voices.items():
                        self.add_lora_voice(name, state=v["state"])
            finally:
                raise e

