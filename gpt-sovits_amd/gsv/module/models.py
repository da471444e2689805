"""Host-side mirror of the reference's `SynthesizerTrn` inference interface
(reference GPT_SoVITS/module/models.py:796-1010), backed by the HIP engine.

`decode` and `extract_latent` keep the reference's argument meaning and return shapes.
All arithmetic runs in libgsv_hip.so; there is no eager/PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Sequence, Union

import torch

from .. import _lib


class SynthesizerTrn:
    _VERSIONS = ("v1", "v2", "v2Pro", "v2ProPlus")
    _FLAVOR = {"v1": 0, "v2": 0, "v2Pro": 0, "v2ProPlus": 0, "v3": 1, "v4": 2}

    def __init__(self, spec_channels, segment_size, inter_channels, hidden_channels, filter_channels, n_heads, n_layers,
                 kernel_size, p_dropout, resblock, resblock_kernel_sizes, resblock_dilation_sizes, upsample_rates,
                 upsample_initial_channel, upsample_kernel_sizes, n_speakers=0, gin_channels=0, use_sdp=True,
                 semantic_frame_rate=None, freeze_quantizer=None, version="v2", device="cuda:0", dtype=torch.float16,
                 n_symbols: Optional[int] = None, **kwargs):
        if version not in self._VERSIONS:
            raise NotImplementedError(f"{type(self).__name__} does not implement SoVITS {version}")
        if str(resblock) != "1":
            raise NotImplementedError("only ResBlock1 generators (reference configs/s2.json)")
        if semantic_frame_rate != "25hz":
            raise NotImplementedError("only the 25hz semantic frame rate (reference configs/s2.json)")
        self.version = version
        self.spec_channels = spec_channels
        self.inter_channels = inter_channels
        self.hidden_channels = hidden_channels
        self.upsample_rates = list(upsample_rates)
        self.semantic_frame_rate = semantic_frame_rate
        self.is_v2pro = version in ("v2Pro", "v2ProPlus")       # reference module/models.py:590, 895
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("gsv SynthesizerTrn runs on an MI355X (cuda/HIP device) only; there is no CPU path")
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        self.dtype = dtype
        if n_symbols is None:
            n_symbols = 322 if version == "v1" else 732     # len(text/symbols.py) / len(text/symbols2.py)
        cfg = _lib.VitsConfig()
        cfg.inter_channels, cfg.hidden_channels, cfg.filter_channels = inter_channels, hidden_channels, filter_channels
        cfg.n_heads, cfg.n_layers, cfg.kernel_size = n_heads, n_layers, kernel_size
        cfg.gin_channels, cfg.n_symbols, cfg.ssl_dim, cfg.n_bins = gin_channels, n_symbols, 768, 1024
        cfg.upsample_initial_channel = upsample_initial_channel
        cfg.n_ups = len(upsample_rates)
        for i, (u, k) in enumerate(zip(upsample_rates, upsample_kernel_sizes)):
            cfg.up_rates[i], cfg.up_kernels[i] = u, k
        cfg.n_resblocks = len(resblock_kernel_sizes)
        for j, (k, ds) in enumerate(zip(resblock_kernel_sizes, resblock_dilation_sizes)):
            cfg.rb_kernels[j] = k
            for c, d in enumerate(ds):
                cfg.rb_dilations[j][c] = d
        cfg.ref_bins = spec_channels if version == "v1" else 704
        cfg.flavor = self._FLAVOR[version]
        cfg.v2pro = int(self.is_v2pro)
        with torch.cuda.device(self.device):
            _lib.init(idx)
            h = C.c_void_p()
            _lib.check(_lib.lib().gsv_vits_create(C.byref(cfg), _lib.dtype_code(dtype), C.byref(h)), "gsv_vits_create")
            self._h = h
            self.stream = torch.cuda.Stream(device=self.device)
        self._cfg = cfg
        self._loaded = False
        self._ref_key = None
        self._ref_hold = None
        self.decode_segments_calls = 0      # test / bench hook: segmented passes run so far

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.lib().gsv_vits_destroy(h)
            except Exception:
                pass
            self._h = None

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = False):
        """Takes the reference checkpoint's `weight` dict (enc_q.* absent or ignored, as with the
        reference's strict=False load, TTS.py:554).  Weight-norm pairs are folded in the library."""
        if self._loaded:
            raise RuntimeError("weights already loaded; create a new SynthesizerTrn")
        l = _lib.lib()
        with torch.cuda.device(self.device):
            _lib.load_tensors(l.gsv_vits_load_tensor, self._h,
                              ((k, v) for k, v in state_dict.items()
                               if torch.is_tensor(v) and not k.startswith("enc_q.") and v.numel()))
            _lib.check(l.gsv_vits_finalize(self._h), "gsv_vits_finalize")
        self._loaded = True
        return self

    # ---- reference audio -------------------------------------------------------------
    def _set_refer(self, refer: Union[torch.Tensor, Sequence[torch.Tensor]], sv_emb=None):
        refs = list(refer) if isinstance(refer, (list, tuple)) else [refer]
        svs = None
        if self.is_v2pro:
            if sv_emb is None:
                raise ValueError("a v2Pro / v2ProPlus model needs sv_emb (one [1, 20480] embedding per reference, sv.py:11-32)")
            svs = list(sv_emb) if isinstance(sv_emb, (list, tuple)) else [sv_emb]
            if len(svs) != len(refs) or any(v.numel() != 20480 for v in svs):
                raise ValueError("sv_emb: expected one [1, 20480] tensor per reference spectrogram")
        elif sv_emb is not None:
            raise ValueError("sv_emb is only used by v2Pro / v2ProPlus models")
        # The key is (address, shape, version) of the caller's tensors; the tensors themselves are held in `_ref_hold`
        # for as long as the key is live, so the caching allocator cannot hand the same address to a different
        # reference spectrogram (the reference recomputes ge from the content on every decode, models.py:966-975).
        key = tuple((r.data_ptr(), tuple(r.shape), r._version) for r in refs + (svs or []))
        if key == self._ref_key:
            return
        keep = [r.to(self.device, torch.float32).contiguous() for r in refs]
        ptrs = (C.c_void_p * len(keep))(*[r.data_ptr() for r in keep])
        frames = (C.c_int * len(keep))(*[int(r.shape[2]) for r in keep])
        bins = int(keep[0].shape[1])
        keep_sv = [v.reshape(-1).to(self.device, torch.float32).contiguous() for v in svs] if svs is not None else None
        # engine stream waits for the conversions above (they run on torch's current stream)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        if svs is None:
            _lib.check(_lib.lib().gsv_vits_set_refer(self._h, ptrs, frames, bins, len(keep),
                                                     C.c_void_p(self.stream.cuda_stream)), "gsv_vits_set_refer")
        else:
            sv_ptrs = (C.c_void_p * len(keep_sv))(*[v.data_ptr() for v in keep_sv])
            _lib.check(_lib.lib().gsv_vits_set_refer_sv(self._h, ptrs, frames, bins, sv_ptrs, len(keep),
                                                        C.c_void_p(self.stream.cuda_stream)), "gsv_vits_set_refer_sv")
        self.stream.synchronize()
        self._ref_key = key
        self._ref_hold = refs + (svs or [])

    def invalidate_refer(self):
        """Forget the cached reference-audio terms (called by TTS.set_prompt_cache / set_ref_audio)."""
        self._ref_key = None
        self._ref_hold = None

    @torch.no_grad()
    def decode(self, codes: torch.Tensor, text: torch.Tensor, refer, noise_scale: float = 0.5, speed: float = 1,
               sv_emb=None, noise: Optional[torch.Tensor] = None, seed: int = 0, align=None) -> torch.Tensor:
        """reference models.py:961-1005: codes [1,1,T] int64, text [1,L] int64, refer = tensor or list of
        [1, bins, Tr] spectrograms -> waveform [1, 1, 2T*prod(upsample_rates)].
        `noise` (optional, [inter, 2T]) injects the randn_like draw of models.py:1000 for parity tests.
        `align` (optional): True = one span over the whole sequence, or spans (code0, n_codes, phone0, n_phones); the phoneme
        alignment of each goes to `self.last_alignment` (see `_align_begin`).  The waveform does not depend on it."""
        if not self._loaded:
            raise RuntimeError("load_state_dict() first")
        if codes.numel() == 0 or text.numel() == 0:
            raise ValueError("decode needs at least one semantic token and one phoneme")
        T = int(codes.shape[-1])
        L = int(text.shape[-1])
        up = math.prod(self.upsample_rates)
        with torch.cuda.device(self.device):
            self._set_refer(refer, sv_emb)
            cd = codes.reshape(-1).to(self.device, torch.int32).contiguous()
            tx = text.reshape(-1).to(self.device, torch.int32).contiguous()
            frames = 2 * T if speed == 1 else int(2 * T / speed) + 1      # models.py:226-228
            nz = None
            if noise is not None:
                nz = noise.reshape(self.inter_channels, frames).to(self.device, torch.float32).contiguous()
            wav = torch.empty(frames * up, dtype=torch.float32, device=self.device)
            # after every conversion above: they are enqueued on torch's current stream, the engine reads on its own
            self.stream.wait_stream(torch.cuda.current_stream(self.device))
            pend = self._align_begin([(0,) + tuple(a) for a in ([(0, T, 0, L)] if align is True else align)]) if align else None
            if align is not None and not align:      # asked for, with no span: no stale result of an earlier call
                self.last_alignment = []
            try:
                _lib.check(_lib.lib().gsv_vits_decode(self._h, cd.data_ptr(), T, tx.data_ptr(), L,
                                                      nz.data_ptr() if nz is not None else None, float(noise_scale),
                                                      float(speed), int(seed) & 0xFFFFFFFFFFFFFFFF, wav.data_ptr(),
                                                      C.c_void_p(self.stream.cuda_stream)), "gsv_vits_decode")
            finally:
                self._align_end(pend)
        return wav.to(self.dtype).view(1, 1, -1)

    last_alignment = None   # [(ends np.int32 [n_phones], score float), ...] of the last call that took `align`, in span order

    def _align_begin(self, spans):
        """Make `spans` [(segment, code0, n_codes, phone0, n_phones), ...] pending for the next engine decode
        (gsv_vits_set_align): span r covers frames 2 code0 .. 2 (code0 + n_codes) of its segment's 50-per-second pre-speed axis
        and the given phones, in the segment's own indices."""
        n = len(spans)
        tab = (_lib.AlignSegSpan * n)(*[_lib.AlignSegSpan(*[int(v) for v in sp]) for sp in spans])
        counts = [int(sp[4]) for sp in spans]
        ends = torch.zeros(max(sum(counts), 1), dtype=torch.int32, device=self.device)
        score = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))     # the two fills above
        _lib.check(_lib.lib().gsv_vits_set_align(self._h, tab, n, ends.data_ptr(), score.data_ptr()), "gsv_vits_set_align")
        return counts, ends, score

    def _align_end(self, pend):
        """after the engine call: wait for its stream (as every decode does), drop a table the call did not reach, and with a
        table fetch the ends and scores that travelled with the audio into `last_alignment`"""
        try:
            self.stream.synchronize()
        finally:
            if pend is not None:
                _lib.lib().gsv_vits_set_align(self._h, None, 0, None, None)
        if pend is None:
            return
        counts, ends, score = pend
        e, sc = ends.cpu().numpy(), score.cpu().numpy()
        out, o = [], 0
        for c, v in zip(counts, sc):
            out.append((e[o:o + c].copy(), float(v)))
            o += c
        self.last_alignment = out

    def segment_gap(self) -> int:
        """Zero frames decode_segments lays between neighbouring segments (gsv_vits_segment_gap): n segments of T_s codes
        take sum(2 T_s) + (n - 1) * segment_gap() frames"""
        return int(_lib.lib().gsv_vits_segment_gap(C.byref(self._cfg)))

    @torch.no_grad()
    def decode_segments(self, codes_list, text_list, voices, seeds, noise_scale: float = 0.5,
                        noise: Optional[Sequence[torch.Tensor]] = None,
                        speeds: Optional[Sequence[float]] = None, align=None) -> List[torch.Tensor]:
        """Segmented decode: segment s = (codes_list[s] [1,1,T_s], text_list[s] [1,L_s], voices[s], seeds[s]) in one
        pass of enc_p, flow and generator (gsv_vits_decode_segments).  A voice is (refer, sv_emb) as taken by `decode`
        (sv_emb None except for v2Pro / v2ProPlus); distinct voices are stored into slots once per call.  `noise`
        (optional) holds one [inter, 2T_s] draw per segment.  Returns one waveform [1, 1, 2T_s * prod(upsample_rates)] per
        segment, what `decode(codes_list[s], text_list[s], *voices[s], noise_scale, seed=seeds[s])` returns.
        `speeds` (optional, one finite positive value per segment; gsv_vits_decode_segments_speed): segment s is decoded at
        `speed=speeds[s]`, so it has F_s = 2T_s frames at speed 1 and int(2T_s / speeds[s]) + 1 otherwise; its noise is
        [inter, F_s] and its waveform [1, 1, F_s * prod(upsample_rates)].
        `align` (optional): one list per segment of spans (code0, n_codes, phone0, n_phones) (True = the whole segment, None /
        empty = none); `self.last_alignment` receives them in segment, then span order.  The waveforms do not depend on it."""
        if not self._loaded:
            raise RuntimeError("load_state_dict() first")
        n = len(codes_list)
        if n == 0 or not (len(text_list) == len(voices) == len(seeds) == n):
            raise ValueError("decode_segments: codes_list, text_list, voices and seeds must have the same non-zero length")
        if noise is not None and len(noise) != n:
            raise ValueError("decode_segments: one noise tensor per segment")
        T = [int(c.shape[-1]) for c in codes_list]
        L = [int(t.shape[-1]) for t in text_list]
        up = math.prod(self.upsample_rates)
        if speeds is None:
            Fs = [2 * t for t in T]
        else:
            if len(speeds) != n:
                raise ValueError("decode_segments: one speed per segment")
            speeds = [float(v) for v in speeds]
            if any(not math.isfinite(v) or v <= 0 for v in speeds):
                raise ValueError("decode_segments: every speed must be finite and positive")
            Fs = [2 * t if v == 1 else int(2 * t / v) + 1 for t, v in zip(T, speeds)]      # as in decode (models.py:226-228)
        self.decode_segments_calls += 1
        with torch.cuda.device(self.device):
            slot_of, slots = {}, []
            for refer, sv_emb in voices:
                refs = list(refer) if isinstance(refer, (list, tuple)) else [refer]
                svl = [] if sv_emb is None else (list(sv_emb) if isinstance(sv_emb, (list, tuple)) else [sv_emb])
                key = tuple(id(r) for r in refs + svl)
                if key not in slot_of:
                    if len(slot_of) >= _lib.VITS_MAX_VOICES:
                        raise ValueError(f"decode_segments: more than {_lib.VITS_MAX_VOICES} distinct voices in one call")
                    self._set_refer(refer, sv_emb)
                    _lib.check(_lib.lib().gsv_vits_store_voice(self._h, len(slot_of)), "gsv_vits_store_voice")
                    slot_of[key] = len(slot_of)
                slots.append(slot_of[key])
            cd = torch.cat([c.reshape(-1) for c in codes_list]).to(self.device, torch.int32).contiguous()
            tx = torch.cat([t.reshape(-1) for t in text_list]).to(self.device, torch.int32).contiguous()
            nz = None
            if noise is not None:
                nz = torch.cat([z.reshape(self.inter_channels, f).to(self.device, torch.float32) for z, f in zip(noise, Fs)],
                               dim=1).contiguous()
            wav = torch.empty(sum(Fs) * up, dtype=torch.float32, device=self.device)
            cl, pl = (C.c_int * n)(*T), (C.c_int * n)(*L)
            vs = (C.c_int * n)(*slots)
            sd = (C.c_uint64 * n)(*[int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds])
            self.stream.wait_stream(torch.cuda.current_stream(self.device))
            nzp = nz.data_ptr() if nz is not None else None
            pend = None
            if align is not None:
                if len(align) != n:
                    raise ValueError("decode_segments: one list of alignment spans per segment")
                spans = [(g,) + tuple(a) for g, al in enumerate(align)
                         for a in ([(0, T[g], 0, L[g])] if al is True else (al or []))]
                pend = self._align_begin(spans) if spans else None
                if not spans:
                    self.last_alignment = []
            try:
                if speeds is None:
                    _lib.check(_lib.lib().gsv_vits_decode_segments(self._h, n, cd.data_ptr(), cl, tx.data_ptr(), pl, vs, sd, nzp,
                                                                   float(noise_scale), wav.data_ptr(),
                                                                   C.c_void_p(self.stream.cuda_stream)), "gsv_vits_decode_segments")
                else:
                    _lib.check(_lib.lib().gsv_vits_decode_segments_speed(self._h, n, cd.data_ptr(), cl, tx.data_ptr(), pl, vs, sd,
                                                                         (C.c_double * n)(*speeds), nzp, float(noise_scale),
                                                                         wav.data_ptr(), C.c_void_p(self.stream.cuda_stream)),
                               "gsv_vits_decode_segments_speed")
            finally:
                self._align_end(pend)
        out = wav.to(self.dtype)
        return [p.view(1, 1, -1) for p in torch.split(out, [f * up for f in Fs])]

    @torch.no_grad()
    def extract_latent(self, x: torch.Tensor) -> torch.Tensor:
        """reference models.py:1007-1010: HuBERT features [1, 768, T50] -> codes [1, 1, T50 // 2] (int64)."""
        if not self._loaded:
            raise RuntimeError("load_state_dict() first")
        T50 = int(x.shape[-1])
        with torch.cuda.device(self.device):
            xs = x.reshape(768, T50).to(self.device, torch.float32).contiguous()
            n = (T50 - 2) // 2 + 1
            out = torch.empty(n, dtype=torch.int32, device=self.device)
            self.stream.wait_stream(torch.cuda.current_stream(self.device))
            _lib.check(_lib.lib().gsv_vits_extract_latent(self._h, xs.data_ptr(), T50, out.data_ptr(),
                                                          C.c_void_p(self.stream.cuda_stream)), "gsv_vits_extract_latent")
            self.stream.synchronize()
        return out.long().view(1, 1, -1)

    @torch.no_grad()
    def extract_latent_many(self, features) -> list:
        """extract_latent for many voices: `features` [1, 768, T50] each -> [1, 1, T50 // 2] int64 codes each, in order.  The
        engine call is issued once per voice on the engine stream, with one wait on the caller's stream before all of them and
        one synchronisation after."""
        if not self._loaded:
            raise RuntimeError("load_state_dict() first")
        outs, held = [], []
        with torch.cuda.device(self.device):
            for x in features:
                T50 = int(x.shape[-1])
                held.append(x.reshape(768, T50).to(self.device, torch.float32).contiguous())
                outs.append(torch.empty((T50 - 2) // 2 + 1, dtype=torch.int32, device=self.device))
            self.stream.wait_stream(torch.cuda.current_stream(self.device))
            for xs, out in zip(held, outs):
                _lib.check(_lib.lib().gsv_vits_extract_latent(self._h, xs.data_ptr(), int(xs.shape[1]), out.data_ptr(),
                                                              C.c_void_p(self.stream.cuda_stream)), "gsv_vits_extract_latent")
            self.stream.synchronize()
        return [out.long().view(1, 1, -1) for out in outs]

    # ---- test / bench hooks -------------------------------------------------------------
    def debug_tensor(self, name: str, numel: int) -> torch.Tensor:
        out = torch.empty(numel, dtype=torch.float32, device=self.device)
        n = C.c_int64(0)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().gsv_vits_debug_tensor(self._h, name.encode(), out.data_ptr(), numel, C.byref(n),
                                                        C.c_void_p(self.stream.cuda_stream)))
            self.stream.synchronize()
        return out[: n.value]

    def last_timing(self):
        a, b = C.c_float(0), C.c_float(0)
        _lib.check(_lib.lib().gsv_vits_last_timing(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value


class SynthesizerTrnV3(SynthesizerTrn):
    """Mirror of the reference's `SynthesizerTrnV3` inference interface (module/models.py:1128-1272) for v3 / v4:
    `decode_encp` (enc_p -> bridge -> nearest x1.875 | x2 -> wns1) in the same HIP engine as v2's enc_p, and `cfm`,
    the flow-matching decoder (`CFM` over `DiT`).  The checkpoint's `cfm.estimator.*` keys go to the DiT engine, the
    rest to the encoder engine.  `cfm` (no counterpart in the reference): build the encoder engine around that loaded `CFM`
    instead of creating and loading a DiT of its own -- the encoder-side engine of a LoRA voice that is served beside the
    base model (TTS.add_lora_voice); load_state_dict then takes the encoder weights only."""
    _VERSIONS = ("v3", "v4")

    def __init__(self, *args, version="v3", device="cuda:0", dtype=torch.float16, dit_kwargs: Optional[dict] = None,
                 cfm: Optional["CFM"] = None, **kwargs):
        super().__init__(*args, version=version, device=device, dtype=dtype, **kwargs)
        self._shared_cfm = cfm is not None
        if cfm is not None:
            if cfm.estimator.dtype != dtype or cfm.estimator.device != self.device:
                raise ValueError("the shared CFM must be on this engine's device, in its dtype")
            self.cfm = cfm
            return
        from ..f5_tts.model.backbones.dit import DiT
        dk = dict(dim=1024, depth=22, heads=16, ff_mult=2, text_dim=512, conv_layers=4)     # models.py:1219-1222
        if dit_kwargs:
            dk.update(dit_kwargs)
        self.cfm = CFM(100, DiT(**dk, device=device, dtype=dtype))

    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = False):
        enc = {k: v for k, v in state_dict.items() if not k.startswith("cfm.")}
        dit = {k: v for k, v in state_dict.items() if k.startswith("cfm.estimator.")}
        super().load_state_dict(enc, strict)
        if not self._shared_cfm:
            self.cfm.estimator.load_state_dict(dit)
        return self

    def decode(self, *a, **k):
        raise NotImplementedError("v3/v4 models synthesise through decode_encp + cfm.inference + a vocoder (TTS.py:1431-1494)")

    @torch.no_grad()
    def decode_encp(self, codes: torch.Tensor, text: torch.Tensor, refer, ge=None, speed: float = 1, align=None):
        """reference models.py:1243-1267: codes [1,1,T], text [1,L], refer [1,bins,Tr] -> (fea [1,512,F], ge).
        `ge` is the handle of the reference audio whose style vector is resident in the engine: pass the value a
        previous call returned (with the same `refer`) to skip recomputing it, exactly like the reference."""
        if not self._loaded:
            raise RuntimeError("load_state_dict() first")
        if codes.numel() == 0 or text.numel() == 0:
            raise ValueError("decode_encp needs at least one semantic token and one phoneme")
        T, L = int(codes.shape[-1]), int(text.shape[-1])
        l = _lib.lib()
        with torch.cuda.device(self.device):
            if ge is None or ge != self._ref_key:
                self._set_refer(refer)
            F_ = l.gsv_vits_encp_frames(self._h, T, float(speed))
            if F_ < 1:
                raise ValueError(f"decode_encp: bad length / speed (T={T}, speed={speed})")
            cd = codes.reshape(-1).to(self.device, torch.int32).contiguous()
            tx = text.reshape(-1).to(self.device, torch.int32).contiguous()
            fea = torch.empty(512, F_, dtype=torch.float32, device=self.device)
            self.stream.wait_stream(torch.cuda.current_stream(self.device))
            # `align`: as in `decode`; the features do not depend on it
            pend = self._align_begin([(0,) + tuple(a) for a in ([(0, T, 0, L)] if align is True else align)]) if align else None
            if align is not None and not align:      # asked for, with no span: no stale result of an earlier call
                self.last_alignment = []
            try:
                _lib.check(l.gsv_vits_decode_encp(self._h, cd.data_ptr(), T, tx.data_ptr(), L, float(speed), fea.data_ptr(),
                                                  C.c_void_p(self.stream.cuda_stream)), "gsv_vits_decode_encp")
            finally:
                self._align_end(pend)
        return fea.to(self.dtype).unsqueeze(0), self._ref_key


class Generator:
    """Host-side mirror of the reference's HiFi-GAN `Generator` used as the v4 mel vocoder
    (reference module/models.py:407-471; constructed in TTS_infer_pack/TTS.py:631-648 with
    initial_channel=100, rates (10,6,2,2,2), kernels (20,12,4,4,4), gin_channels=0, is_bias=True)."""

    def __init__(self, initial_channel, resblock, resblock_kernel_sizes, resblock_dilation_sizes, upsample_rates,
                 upsample_initial_channel, upsample_kernel_sizes, gin_channels=0, is_bias=False, device="cuda:0",
                 dtype=torch.float16):
        from .vocoder import _VocoderEngine
        if str(resblock) != "1":
            raise NotImplementedError("only ResBlock1 generators")
        if gin_channels != 0:
            raise NotImplementedError("the conditioned generator is part of SynthesizerTrn.decode")
        self._e = _VocoderEngine(0, initial_channel, upsample_initial_channel, upsample_rates, upsample_kernel_sizes,
                                 resblock_kernel_sizes, resblock_dilation_sizes, bias_at_final=is_bias, tanh_at_final=True,
                                 snake_logscale=False, device=device, dtype=dtype)

    def load_state_dict(self, sd, strict=True):
        self._e.load_state_dict(sd, strict)
        return self

    def remove_weight_norm(self):   # folded at load
        return self

    def eval(self):
        return self

    def __call__(self, x, g=None):
        if g is not None:
            raise NotImplementedError("conditioning input g")
        return self._e(x)

    def forward_segments(self, mels):
        """mels[s] [1, initial_channel, F_s] -> waveforms [1, 1, F_s * prod(upsample_rates)], each what self(mels[s]) gives, from
        one generator pass over all of them (no counterpart in the reference, which vocodes one mel per call)"""
        return self._e.forward_segments(mels)

    def segment_gap(self) -> int:
        return self._e.segment_gap()


def cfg_guided(rate) -> bool:
    """Is classifier-free guidance active at this rate?  The reference's test `rate > 1e-5` (models.py:1063), taken in fp32
    as the engine takes it (`cfg_rate > 1e-5f` on the float that crosses the C ABI), so the host mirror, the pass planner and
    the engine agree on every rate.  False for NaN."""
    return C.c_float(rate).value > C.c_float(1e-5).value


class CFM:
    """Mirror of the reference's `CFM` (module/models.py:1013-1085): `inference` integrates the flow-matching ODE with
    `n_timesteps` Euler steps over the `DiT` estimator, entirely inside the HIP library (`gsv_cfm_inference`).

    `noise` (not in the reference signature) pins the `torch.randn` draw of models.py:1030 for parity tests; left
    None, the draw happens on the device from `seed`.

    Classifier-free guidance (`inference_cfg_rate` > 1e-5, the reference's test, models.py:1063) is `inference_guided` /
    `inference_rows(..., inference_cfg_rate=r)`: every row gets an unconditioned twin in the same DiT pass
    (`gsv_cfm_inference_guided`).  `inference` is the unguided entry and refuses a positive rate; `inference_guided` is the
    guided one.
    """
    GOLDEN = 0x9E3779B97F4A7C15     # row b of `inference(seed=s)` draws with the key s + GOLDEN * b

    def __init__(self, in_channels, dit):
        self.in_channels = in_channels
        self.estimator = dit
        self.sigma_min = 1e-6

    @classmethod
    def row_seed(cls, seed: int, b: int) -> int:
        """the 64-bit noise key of row b of a batch drawn with `seed`: what gsv_cfm_inference gives its row b"""
        return (int(seed) + cls.GOLDEN * int(b)) & 0xFFFFFFFFFFFFFFFF

    def _check_mu_noise(self, mu, noise):
        """the checks `inference` and `inference_rows` share -> (B, T) of mu [B, T, text_dim]"""
        dit = self.estimator
        if not dit._loaded:
            raise RuntimeError("DiT.load_state_dict() first")
        if mu.dim() != 3 or mu.shape[2] != dit.text_dim or mu.shape[1] < 1:
            raise ValueError(f"expected mu of shape [B, T>=1, {dit.text_dim}], got {tuple(mu.shape)}")
        B, T = int(mu.shape[0]), int(mu.shape[1])
        if noise is not None and tuple(noise.shape) != (B, self.in_channels, T):
            raise ValueError(f"noise must have shape {(B, self.in_channels, T)}")
        return B, T

    def _launch(self, mu, prompts, noise, call):
        """Around one C call on the DiT's stream: fp32 contiguous copies of mu, the prompts and the noise on its device, `out`
        [B, in_channels, T] fp32, the wait for torch's current stream, `call(m, ps, nz_ptr, out, stream)`, the synchronize;
        returns `out` in mu's dtype (fp16 / fp32, anything else fp32)."""
        dit = self.estimator
        dev = dit.device
        with torch.cuda.device(dev):
            m = mu.to(dev, torch.float32).contiguous()
            ps = [p.to(dev, torch.float32).contiguous() for p in prompts]
            nz = noise.to(dev, torch.float32).contiguous() if noise is not None else None
            out = torch.empty(int(mu.shape[0]), self.in_channels, int(mu.shape[1]), dtype=torch.float32, device=dev)
            dit.stream.wait_stream(torch.cuda.current_stream(dev))
            call(m, ps, nz.data_ptr() if nz is not None else None, out, C.c_void_p(dit.stream.cuda_stream))
            dit.stream.synchronize()
        return out.to(mu.dtype if mu.dtype in (torch.float16, torch.float32) else torch.float32)

    def add_adapter(self, adapter, rank, alpha=None) -> int:
        """A LoRA voice's adapter into the estimator (DiT.add_adapter) -> its slot, for `adapters=` below"""
        return self.estimator.add_adapter(adapter, rank, alpha)

    def remove_adapter(self, slot: int) -> None:
        self.estimator.remove_adapter(slot)

    def _adapter_slots(self, adapters, B):
        """`adapters` (B slots or None entries, or None) -> B ints, -1 = the base model, or None when no row is adapted"""
        if adapters is None:
            return None
        if len(adapters) != B:
            raise ValueError(f"expected {B} adapters, one per row of mu (None = the base model), got {len(adapters)}")
        slots = [-1 if a is None else int(a) for a in adapters]
        for b, a in enumerate(slots):
            if a != -1 and a not in self.estimator._adapters:
                raise ValueError(f"row {b}: no adapter in slot {a}")
        return slots if any(a >= 0 for a in slots) else None

    @torch.no_grad()
    def inference(self, mu, x_lens, prompt, n_timesteps, temperature=1.0, inference_cfg_rate=0, noise=None, seed=0, adapters=None):
        """mu [B, T, text_dim]; x_lens unused (as in the reference); prompt [B, in_channels, Tp] -> [B, in_channels, T].
        `adapters` (B slots or None entries) with a slot among them: the rows entry, as `inference_guided` takes it."""
        if inference_cfg_rate > 1e-5:
            raise NotImplementedError("CFM.inference is the unguided entry (every caller in the reference passes "
                                      "inference_cfg_rate=0, TTS.py:1351, inference_webui.py:937); classifier-free guidance "
                                      "is CFM.inference_guided")
        B, T = self._check_mu_noise(mu, noise)
        if prompt.dim() != 3 or prompt.shape[0] not in (1, B) or prompt.shape[1] != self.in_channels or prompt.shape[2] > T:
            raise ValueError(f"expected prompt of shape [{B} or 1, {self.in_channels}, Tp<={T}], got {tuple(prompt.shape)}")
        if self._adapter_slots(adapters, B) is not None:
            return self.inference_guided(mu, x_lens, prompt, n_timesteps, temperature=temperature, noise=noise, seed=seed,
                                         adapters=adapters)
        if prompt.shape[0] != B:           # one prompt broadcast over the batch (models.py:1036 assigns it into every row)
            prompt = prompt.expand(B, -1, -1)
        Tp = int(prompt.shape[2])

        def call(m, ps, nz, out, stream):
            _lib.check(_lib.lib().gsv_cfm_inference(self.estimator._h, m.data_ptr(), ps[0].data_ptr() if Tp else None, B, T, Tp,
                                                    int(n_timesteps), nz, float(temperature), int(seed), out.data_ptr(), stream),
                       "gsv_cfm_inference")
        return self._launch(mu, [prompt], noise, call)

    @torch.no_grad()
    def inference_guided(self, mu, x_lens, prompt, n_timesteps, temperature=1.0, inference_cfg_rate=0, noise=None, seed=0,
                         adapters=None):
        """The reference's `CFM.inference(..., inference_cfg_rate=r)` with classifier-free guidance (models.py:1063-1081);
        arguments as `inference`.  r > 1e-5: the rows entry with uniform prompts and seeds[b] = row_seed(seed, b), so the
        noise is the unguided call's.  r <= 1e-5 (zero and negative rates included) is `inference` itself.
        `adapters` (B slots or None entries): as in `inference_rows`; with an adapted row every rate takes the rows entry."""
        if not math.isfinite(inference_cfg_rate):
            raise ValueError(f"inference_cfg_rate must be finite, got {inference_cfg_rate}")
        if adapters is not None and mu.dim() == 3:
            adapters = self._adapter_slots(adapters, int(mu.shape[0]))
        if not cfg_guided(inference_cfg_rate) and adapters is None:
            return self.inference(mu, x_lens, prompt, n_timesteps, temperature=temperature, noise=noise, seed=seed)
        B = int(mu.shape[0]) if mu.dim() == 3 else 0
        if prompt.dim() != 3 or prompt.shape[0] not in (1, B):
            raise ValueError(f"expected prompt of shape [{B} or 1, {self.in_channels}, Tp], got {tuple(prompt.shape)}")
        return self.inference_rows(mu, [prompt[b:b + 1] if prompt.shape[0] == B else prompt for b in range(B)], n_timesteps,
                                   temperature=temperature, noise=noise, seeds=[self.row_seed(seed, b) for b in range(B)],
                                   inference_cfg_rate=inference_cfg_rate, adapters=adapters)

    @torch.no_grad()
    def inference_rows(self, mu, prompts, n_timesteps, temperature=1.0, noise=None, seeds=None, inference_cfg_rate=0, adapters=None):
        """`inference` for B rows that each have their own prompt (`gsv_cfm_inference_rows`): mu [B, T, text_dim]; prompts a
        list of B tensors [1, in_channels, Tp_b], 0 <= Tp_b <= T -> [B, in_channels, T], row b's first Tp_b frames zero.
        `seeds` (B ints) are the rows' own noise keys, taken as they are: row b of `inference(seed=s)` is seeds[b] =
        row_seed(s, b) here.  `noise` [B, in_channels, T] pins the draw instead.  `inference_cfg_rate` > 1e-5
        guides every row with that rate (`gsv_cfm_inference_guided`, 2 B DiT rows); the noise of a row does not depend on it.
        `adapters` (B entries: a slot `add_adapter` returned, or None = the base model): row b runs the DiT with that LoRA
        adapter (`gsv_cfm_inference_adapted`; a guided row's twin takes the row's).  None, or no slot among them, is the
        call without the keyword.
        `n_timesteps` and `inference_cfg_rate` may each be a list / tuple of B values, one per row: the rows then run through a
        flow-matching session opened and closed here (`open_session`), every row with its own step count and rate; row b
        equals the row of a call with its own scalars.  Scalars keep the one-shot entries above and their launches.  A session
        holds at most 64 DiT rows (a guided row counts 2): the sequence form raises ValueError above that, the scalar form has no
        such limit."""
        B, T = self._check_mu_noise(mu, noise)
        if isinstance(n_timesteps, (list, tuple)) or isinstance(inference_cfg_rate, (list, tuple)):
            return self._inference_rows_session(mu, prompts, n_timesteps, temperature, noise, seeds, inference_cfg_rate, adapters)
        slots = self._adapter_slots(adapters, B)
        if B < 1 or len(prompts) != B:
            raise ValueError(f"expected {B} >= 1 prompts, one per row of mu, got {len(prompts)}")
        for b, p in enumerate(prompts):
            if p.dim() != 3 or p.shape[0] != 1 or p.shape[1] != self.in_channels or p.shape[2] > T:
                raise ValueError(f"expected prompt {b} of shape [1, {self.in_channels}, Tp<={T}], got {tuple(p.shape)}")
        if not math.isfinite(inference_cfg_rate):
            raise ValueError(f"inference_cfg_rate must be finite, got {inference_cfg_rate}")
        if noise is None and seeds is None:
            raise ValueError("inference_rows needs `noise` or `seeds`")
        if seeds is not None and len(seeds) != B:
            raise ValueError(f"expected {B} seeds, got {len(seeds)}")

        def call(m, ps, nz, out, stream):
            ptrs = (C.c_void_p * B)(*[p.data_ptr() if p.shape[2] else None for p in ps])
            tps = (C.c_int * B)(*[int(p.shape[2]) for p in ps])
            sd = (C.c_uint64 * B)(*[int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds]) if seeds is not None else None
            h, lib = self.estimator._h, _lib.lib()
            if slots is not None:
                _lib.check(lib.gsv_cfm_inference_adapted(h, m.data_ptr(), ptrs, tps, (C.c_int * B)(*slots), B, T, int(n_timesteps), nz,
                                                         sd, float(temperature), float(inference_cfg_rate), out.data_ptr(), stream),
                           "gsv_cfm_inference_adapted")
            elif cfg_guided(inference_cfg_rate):
                _lib.check(lib.gsv_cfm_inference_guided(h, m.data_ptr(), ptrs, tps, B, T, int(n_timesteps), nz, sd, float(temperature),
                                                        float(inference_cfg_rate), out.data_ptr(), stream), "gsv_cfm_inference_guided")
            else:
                _lib.check(lib.gsv_cfm_inference_rows(h, m.data_ptr(), ptrs, tps, B, T, int(n_timesteps), nz, sd, float(temperature),
                                                      out.data_ptr(), stream), "gsv_cfm_inference_rows")
        return self._launch(mu, prompts, noise, call)

    def _inference_rows_session(self, mu, prompts, n_timesteps, temperature, noise, seeds, rates, adapters):
        """`inference_rows` with per-row step counts / rates: one session, every row admitted at once, stepped to the largest count"""
        B, T = int(mu.shape[0]), int(mu.shape[1])
        steps = [int(n) for n in n_timesteps] if isinstance(n_timesteps, (list, tuple)) else [int(n_timesteps)] * B
        rates = [float(r) for r in rates] if isinstance(rates, (list, tuple)) else [float(rates)] * B
        if len(steps) != B or len(rates) != B:
            raise ValueError(f"expected {B} step counts and {B} rates, one per row of mu, got {len(steps)} and {len(rates)}")
        cap = sum(2 if cfg_guided(r) else 1 for r in rates)
        if cap > _lib.CFM_SESSION_MAX_ROWS:
            raise ValueError(f"{cap} DiT rows (a guided row counts 2) exceed the {_lib.CFM_SESSION_MAX_ROWS} of one session")
        sess = self.open_session(cap, T, temperature)
        try:
            slots = sess.admit(mu, prompts, steps, rates, seeds=seeds, noise=noise, adapters=adapters)
            sess.step(max(steps))
            out = torch.stack([sess.fetch(sl) for sl in slots])
        finally:
            sess.close()
        return out.to(mu.dtype if mu.dtype in (torch.float16, torch.float32) else torch.float32)

    def open_session(self, rows_cap, T, temperature=1.0) -> "CFMSession":
        """A flow-matching session (`gsv_cfm_session_*`) for rows of T frames: rows with their own step count, guidance rate and
        LoRA slot enter (`admit`) and leave (`fetch`, `release`) between Euler steps (`step`).  `rows_cap` counts DiT rows: a guided
        row (`cfg_guided(rate)`) takes two; at most 64 (`_lib.CFM_SESSION_MAX_ROWS`), more is an error of the engine.  One session
        per DiT at a time; the one-shot entries raise while it is open, and so does `remove_adapter` of a slot a live row uses."""
        return CFMSession(self, rows_cap, T, temperature)


class CFMSession:
    """One open flow-matching session of a `CFM` (see `CFM.open_session`).  Every method issues its launches on the DiT's
    stream and waits for them, so the tensors given to `admit` may go afterwards and `fetch` returns a finished tensor."""
    FREE, LIVE, FINISHED = 0, 1, 2

    def __init__(self, cfm, rows_cap, T, temperature=1.0):
        dit = cfm.estimator
        if not dit._loaded:
            raise RuntimeError("DiT.load_state_dict() first")
        self.cfm, self.rows_cap, self.T = cfm, int(rows_cap), int(T)
        self._open = False
        with torch.cuda.device(dit.device):
            dit.stream.wait_stream(torch.cuda.current_stream(dit.device))
            _lib.check(_lib.lib().gsv_cfm_session_begin(dit._h, self.rows_cap, self.T, float(temperature),
                                                        C.c_void_p(dit.stream.cuda_stream)), "gsv_cfm_session_begin")
        self._open = True

    @property
    def state(self):
        """per slot (state, steps taken, n_steps), state one of FREE / LIVE / FINISHED: host bookkeeping, no device wait"""
        buf = (C.c_int32 * (3 * self.rows_cap))()
        _lib.check(_lib.lib().gsv_cfm_session_state(self.cfm.estimator._h, buf), "gsv_cfm_session_state")
        n = self.rows_cap
        return [(buf[s], buf[n + s], buf[2 * n + s]) for s in range(n)]

    def free_slots(self):
        return [s for s, st in enumerate(self.state) if st[0] == self.FREE]

    @torch.no_grad()
    def admit(self, mu, prompts, n_timesteps, inference_cfg_rate, seeds=None, noise=None, adapters=None, slots=None):
        """Admits the B rows of mu [B, T, text_dim] (prompts, seeds, noise, adapters as `CFM.inference_rows`); `n_timesteps` and
        `inference_cfg_rate` are a scalar or one value per row.  `slots` (B free slots) defaults to the lowest free ones.
        Returns the slots.  The engine refuses, before it launches anything, an admission that does not fit `rows_cap`."""
        cfm, dit = self.cfm, self.cfm.estimator
        B, T = cfm._check_mu_noise(mu, noise)
        if T != self.T:
            raise ValueError(f"the session holds rows of {self.T} frames, got {T}")
        steps = [int(n) for n in n_timesteps] if isinstance(n_timesteps, (list, tuple)) else [int(n_timesteps)] * B
        rates = [float(r) for r in inference_cfg_rate] if isinstance(inference_cfg_rate, (list, tuple)) else [float(inference_cfg_rate)] * B
        if len(steps) != B or len(rates) != B or len(prompts) != B:
            raise ValueError(f"expected {B} prompts, step counts and rates, one per row of mu")
        for b, p in enumerate(prompts):
            if p is not None and (p.dim() != 3 or p.shape[0] != 1 or p.shape[1] != cfm.in_channels):
                raise ValueError(f"expected prompt {b} of shape [1, {cfm.in_channels}, Tp], got {tuple(p.shape)}")
        if noise is None and seeds is None:
            raise ValueError("admit needs `noise` or `seeds`")
        if seeds is not None and len(seeds) != B:
            raise ValueError(f"expected {B} seeds, got {len(seeds)}")
        ad = cfm._adapter_slots(adapters, B)
        if slots is None:
            slots = self.free_slots()[:B]
            if len(slots) < B:
                raise RuntimeError(f"libgsv_hip gsv_cfm_session_admit refused: {B} rows, {len(slots)} free slots")
        slots = [int(s) for s in slots]
        dev = dit.device
        with torch.cuda.device(dev):
            m = mu.to(dev, torch.float32).contiguous()
            ps = [None if p is None else p.to(dev, torch.float32).contiguous() for p in prompts]
            nz = noise.to(dev, torch.float32).contiguous() if noise is not None else None
            ptrs = (C.c_void_p * B)(*[p.data_ptr() if p is not None and p.shape[2] else None for p in ps])
            tps = (C.c_int * B)(*[0 if p is None else int(p.shape[2]) for p in ps])
            sd = (C.c_uint64 * B)(*[int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds]) if seeds is not None else None
            dit.stream.wait_stream(torch.cuda.current_stream(dev))
            _lib.check(_lib.lib().gsv_cfm_session_admit(dit._h, B, (C.c_int32 * B)(*slots), m.data_ptr(), ptrs, tps,
                                                        (C.c_int * B)(*ad) if ad is not None else None, (C.c_int * B)(*steps),
                                                        (C.c_float * B)(*rates), nz.data_ptr() if nz is not None else None, sd,
                                                        C.c_void_p(dit.stream.cuda_stream)), "gsv_cfm_session_admit")
            dit.stream.synchronize()
        return slots

    @torch.no_grad()
    def step(self, k=1):
        """k Euler steps of every live row -> the slots that finished during the call (ascending)"""
        dit = self.cfm.estimator
        before = self.state
        with torch.cuda.device(dit.device):
            _lib.check(_lib.lib().gsv_cfm_session_step(dit._h, int(k), C.c_void_p(dit.stream.cuda_stream)), "gsv_cfm_session_step")
            dit.stream.synchronize()
        after = self.state
        return [s for s in range(self.rows_cap) if before[s][0] == self.LIVE and after[s][0] == self.FINISHED]

    @torch.no_grad()
    def fetch(self, slot, out=None):
        """a finished row -> [in_channels, T] fp32, its prompt frames zero; frees the slot"""
        dit = self.cfm.estimator
        with torch.cuda.device(dit.device):
            if out is None:
                out = torch.empty(self.cfm.in_channels, self.T, dtype=torch.float32, device=dit.device)
            dit.stream.wait_stream(torch.cuda.current_stream(dit.device))
            _lib.check(_lib.lib().gsv_cfm_session_fetch(dit._h, int(slot), out.data_ptr(), C.c_void_p(dit.stream.cuda_stream)),
                       "gsv_cfm_session_fetch")
            dit.stream.synchronize()
        return out

    @torch.no_grad()
    def fetch_mel(self, slots, col0, out, lo, hi):
        """Finished rows straight into the vocoder's layout, one launch and one stream wait for all of them: the generated frames
        [Tp, T) of slot slots[i], de-normalised as `denorm_spec` does it (((x + 1) / 2) * (hi - lo) + lo), go to columns
        [col0[i], col0[i] + T - Tp) of `out`, a contiguous fp32 matrix [in_channels, ld] on the DiT's device (a leading dimension
        of 1 is allowed).  The bits are those of denorm_spec(fetch(slot)[:, Tp:]).  Frees the slots.  The
        engine refuses, before it launches anything, a slot that is not FINISHED or given twice, a negative col0 and a range
        that does not fit `out`; the ranges are not checked against each other."""
        dit = self.cfm.estimator
        slots, col0 = [int(s) for s in slots], [int(c) for c in col0]
        if len(slots) != len(col0):
            raise ValueError(f"{len(slots)} slots, {len(col0)} columns")
        m = out[0] if out.dim() == 3 and out.shape[0] == 1 else out
        if m.dim() != 2 or m.shape[0] != self.cfm.in_channels or m.dtype != torch.float32 or not m.is_cuda or not m.is_contiguous():
            raise ValueError(f"out must be a contiguous fp32 matrix [{self.cfm.in_channels}, ld] on {dit.device}")
        n = len(slots)
        with torch.cuda.device(dit.device):
            dit.stream.wait_stream(torch.cuda.current_stream(dit.device))
            _lib.check(_lib.lib().gsv_cfm_session_fetch_mel(dit._h, n, (C.c_int32 * max(1, n))(*slots), (C.c_int * max(1, n))(*col0),
                                                            int(m.shape[1]), float(lo), float(hi),
                                                            m.data_ptr(), C.c_void_p(dit.stream.cuda_stream)), "gsv_cfm_session_fetch_mel")
            dit.stream.synchronize()
        return out

    def release(self, slots):
        """drops live or finished rows (cancellation); the others are not touched"""
        slots = [int(s) for s in slots]
        _lib.check(_lib.lib().gsv_cfm_session_release(self.cfm.estimator._h, len(slots), (C.c_int32 * max(1, len(slots)))(*slots)),
                   "gsv_cfm_session_release")

    def close(self):
        if self._open:
            self._open = False
            _lib.check(_lib.lib().gsv_cfm_session_end(self.cfm.estimator._h), "gsv_cfm_session_end")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
