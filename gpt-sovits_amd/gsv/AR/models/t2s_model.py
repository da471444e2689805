"""Host-side mirror of the reference's `Text2SemanticDecoder` inference interface
(reference GPT_SoVITS/AR/models/t2s_model.py:260-935), backed by the HIP engine.

Same entry points, argument meaning and return values as the reference:
`infer_panel_batch_infer` (:583), `infer_panel_naive_batched` (:781), `infer_panel_naive` (:814),
`infer_panel` (:920).  All arithmetic (embeddings, prefill, KV-cached decode, sampling, EOS /
early-stop bookkeeping) runs in libgsv_hip.so; this class only packs inputs and unpacks
outputs.  There is no eager/PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import math
import warnings
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from ... import _lib


def _sine_pe(n_pos: int, dim: int) -> torch.Tensor:
    """Position table, computed exactly as the reference does on the host
    (AR/modules/embedding.py:54-72) so the fp32 engine sees bit-identical values."""
    position = torch.arange(0, n_pos, dtype=torch.float32).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, dim, 2, dtype=torch.float32) * -(math.log(10000.0) / dim))
    pe = torch.zeros(n_pos, dim)
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe


def _host_nonzero(t: torch.Tensor) -> bool:
    """any(t != 0) for a host tensor without a torch dispatch (bfloat16 has no numpy view: torch then)"""
    try:
        return bool(np.any(t.detach().numpy()))
    except (TypeError, RuntimeError):
        return bool(t.any())


def admit_count(free: int, queued: int, live: int, admit_min: int) -> int:
    """The admission policy of a decode session: how many rows of the queue go into free slots now.  Rows wait until
    `admit_min` slots are free, so that a prefill is shared by several rows -- unless fewer than that are left in the queue
    (its tail) or nothing is decoding (the engine would otherwise idle)."""
    if queued <= 0 or free <= 0:
        return 0
    if free >= min(admit_min, queued) or live == 0:
        return min(free, queued)
    return 0


def plan_continuous(lengths: Sequence[int], slots: int, chunk: int, admit_min: Optional[int] = None):
    """The schedule `infer_panel_continuous` follows for a queue whose row i needs lengths[i] further steps after its step 0
    (0: it ends at its admission), as a pure function: a list of ("admit", [(row, slot), ...]) and
    ("advance", chunk, [rows reported finished, in slot order]) events.  Rows are admitted in the order given, into the lowest
    free slots; a slot is free again once the advance that saw its row finish has returned."""
    if slots < 1 or chunk < 1:
        raise ValueError("slots and chunk must be >= 1")
    admit_min = max(1, slots // 4) if admit_min is None else int(admit_min)
    if admit_min < 1:
        raise ValueError("admit_min must be >= 1")
    trace = []
    owner: List[Optional[int]] = [None] * slots      # row in each slot
    left: List[int] = [0] * slots
    q, n = 0, len(lengths)
    while q < n or any(o is not None for o in owner):
        free = [s for s in range(slots) if owner[s] is None]
        k = admit_count(len(free), n - q, slots - len(free), admit_min)
        if k:
            pairs = []
            for s in free[:k]:
                owner[s], left[s] = q, int(lengths[q])
                pairs.append((q, s))
                q += 1
            trace.append(("admit", pairs))
        done = []
        for s in range(slots):
            if owner[s] is None:
                continue
            left[s] -= min(chunk, left[s])
            if left[s] == 0:
                done.append(owner[s])
                owner[s] = None
        trace.append(("advance", chunk, done))
    return trace


def row_limit_tuples(row_limits, needs, max_seq):
    """The per-row limits as the engine takes them.  row_limits: [(eos_mask_steps, early_stop_num | None, max_steps)], needs:
    the positions each row's text + prompt use (+ 2).  A row's budget is min(wanted_b, max_seq - need_b), wanted_b =
    min(max_steps_b, early_stop_num_b + 1): where the arena is the smaller bound it becomes the row's max_steps.  Returns
    (tuples, budgets, whether the arena bounds any row)."""
    out, budgets, short = [], [], False
    for (eos, es, ms), need in zip(row_limits, needs):
        es = -1 if es is None else int(es)
        want = int(ms) if es == -1 else min(int(ms), es + 1)
        b = min(want, max_seq - need)
        short = short or b < want
        out.append((int(eos), es if es != -1 and es + 1 <= b else -1, max(b, 1)))
        budgets.append(b)
    return out, budgets, short


def row_sampling_array(rows):
    """[(top_k | None, top_p | None, temperature, repetition_penalty)] as the gsv_row_sampling_t array the engine takes"""
    return (_lib.RowSampling * len(rows))(*[_lib.RowSampling(int(k) if k is not None else 0, float(p if p is not None else 1.0),
                                                             float(t), float(rp)) for k, p, t, rp in rows])


def row_limits_array(limits):
    """row_limit_tuples' tuples as the gsv_row_limits_t array the engine takes"""
    return (_lib.RowLimits * len(limits))(*[_lib.RowLimits(e, es, ms, 0) for e, es, ms in limits])


class T2SSession:
    """An open decode session of a Text2SemanticDecoder (gsv_t2s_session_*): `slots` rows of its K/V arena that are admitted,
    advanced a chunk of steps at a time and admitted again when their row has finished.  Use as a context manager."""

    def __init__(self, dec: "Text2SemanticDecoder", slots, top_k, top_p, temperature, repetition_penalty, early_stop_num,
                 eos_mask_steps, max_steps, row_sampling=False, force=False, dump_logits=False, logprobs=False, row_limits=False):
        if not dec._loaded:
            raise RuntimeError("load_state_dict() first")
        self.dec, self.slots, self.per_row = dec, int(slots), bool(row_sampling)
        self.row_limits = bool(row_limits)
        self.scalars = (int(eos_mask_steps), -1 if early_stop_num is None else int(early_stop_num))
        dev = dec.device
        wanted = max_steps if early_stop_num in (-1, None) else min(max_steps, int(early_stop_num) + 1)
        self.budget = int(wanted)
        self._row_budget = [self.budget] * self.slots              # the budget of the row in each slot (its own with limits)
        self._owner: List[Optional[int]] = [None] * self.slots     # ticket of the row in each slot
        self._prompt: List[Optional[torch.Tensor]] = [None] * self.slots
        self._next_ticket = 0
        self.modes: List[int] = []          # decode_info mode of every advance that ran a step
        self.logits: Dict[int, torch.Tensor] = {}   # dump_logits: ticket -> [steps run][vocab]
        self.logprobs: Dict[int, torch.Tensor] = {} # logprobs: ticket -> [idx + 1], the taken tokens' log-probabilities
        self.cut: Dict[int, bool] = {}              # logprobs: ticket -> the step budget ended the row, not EOS
        self.adopt: List[tuple] = []        # (rows, device ms, K/V bytes) of every admission
        self.history: List[tuple] = []      # (ticket, slot) of every admitted row
        self._open = False
        with torch.cuda.device(dev):
            self.out_tokens = torch.zeros(self.slots, self.budget, dtype=torch.int32, device=dev)
            self.out_len = torch.full((self.slots,), -1, dtype=torch.int32, device=dev)
            self.force = torch.zeros(self.slots, self.budget, dtype=torch.int32, device=dev) if force else None
            self.dump = torch.zeros(self.budget, self.slots, dec.vocab_size, dtype=torch.float32, device=dev) if dump_logits else None
            self.logp = torch.full((self.slots, self.budget), float("nan"), dtype=torch.float32, device=dev) if logprobs else None
            sp = _lib.SamplingParams(int(top_k) if top_k is not None else 0, float(top_p if top_p is not None else 1.0),
                                     float(temperature), float(repetition_penalty),
                                     -1 if early_stop_num is None else int(early_stop_num), int(eos_mask_steps),
                                     self.budget, 0)
            torch.cuda.current_stream(dev).synchronize()
            l = _lib.lib()
            if force or dump_logits:
                _lib.check(l.gsv_t2s_set_debug(dec._h, self.force.data_ptr() if force else None,
                                               self.dump.data_ptr() if dump_logits else None, None), "gsv_t2s_set_debug")
            if logprobs:
                _lib.check(l.gsv_t2s_set_logprobs(dec._h, self.logp.data_ptr()), "gsv_t2s_set_logprobs")
            _lib.check(l.gsv_t2s_session_begin(dec._h, C.byref(sp), self.slots, int(self.per_row), self.out_tokens.data_ptr(),
                                               self.out_len.data_ptr()), "gsv_t2s_session_begin")
        self._open = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        if self._open:
            self._open = False
            _lib.check(_lib.lib().gsv_t2s_session_end(self.dec._h), "gsv_t2s_session_end")

    @property
    def free(self) -> List[int]:
        """slots that hold no row (a finished row keeps its slot until an advance has reported it)"""
        return [s for s in range(self.slots) if self._owner[s] is None]

    @property
    def live(self) -> int:
        return sum(o is not None for o in self._owner)

    def admit(self, rows: Sequence[dict], slots: Optional[Sequence[int]] = None) -> List[int]:
        """rows: dict(x, bert, prompt, key=(seed, row), sampling=None[, force=tokens][, limits=(eos_mask_steps, early_stop_num,
        max_steps)]); each goes into the next free slot (or slots[i]) and has run its step 0 when this returns.  In a session
        opened with row_limits=True a row may bring limits, which replace the session's three for it (its budget also bounded by
        the K/V arena), and prompt=None: a prompt-free row.  Returns one ticket per row."""
        dec, dev, n = self.dec, self.dec.device, len(rows)
        if slots is None:
            slots = self.free[:n]
            if len(slots) < n:
                raise ValueError(f"{n} rows for {len(slots)} free slots")
        slots = [int(s) for s in slots]
        if len(slots) != n:
            raise ValueError(f"{len(slots)} slots for {n} rows")
        if self.per_row and any(r.get("sampling") is None for r in rows):
            raise ValueError("the session samples per row: every row needs a sampling tuple")
        l = _lib.lib()
        with torch.cuda.device(dev):
            lens = [int(r["x"].shape[-1]) for r in rows]
            prompts = [torch.zeros(0, dtype=torch.int64) if r.get("prompt") is None else r["prompt"].reshape(-1) for r in rows]
            plens = [int(p_.shape[0]) for p_ in prompts]
            limits, budgets = None, [self.budget] * n
            if any(r.get("limits") is not None for r in rows) or min(plens) < 1:
                if not self.row_limits:
                    raise ValueError("limits or a prompt-free row in a session opened without row_limits=True")
                mine = [r["limits"] if r.get("limits") is not None else (self.scalars[0], self.scalars[1], self.budget) for r in rows]
                needs = [a + b + 2 for a, b in zip(lens, plens)]
                limits, budgets, _ = row_limit_tuples(mine, needs, dec.max_seq)
                if min(budgets) < 1:
                    raise ValueError(f"sequence of {needs[budgets.index(min(budgets))]} positions does not fit max_seq={dec.max_seq}")
                if max(budgets) > self.budget:
                    raise ValueError(f"a row's budget of {max(budgets)} steps exceeds the session's {self.budget}")
            phones = torch.cat([r["x"].reshape(-1) for r in rows]).to(dev, torch.int32).contiguous()
            bert_dev = dec._bert_rows([r.get("bert") for r in rows], lens)
            pr = torch.cat([p_.to(dev, torch.int32) for p_ in prompts]).contiguous()
            if self.force is not None:
                for r, s in zip(rows, slots):
                    if r.get("force") is not None and 0 <= s < self.slots:
                        f = r["force"].reshape(-1).to(dev, torch.int32)[:self.budget]
                        self.force[s].zero_()
                        self.force[s, :f.shape[0]] = f
            dec.stream.wait_stream(torch.cuda.current_stream(dev))
            torch.cuda.current_stream(dev).synchronize()
            slots_h, lens_h, plens_h = (C.c_int32 * n)(*slots), (C.c_int32 * n)(*lens), (C.c_int32 * n)(*plens)
            seeds_h = (C.c_uint64 * n)(*[int(r["key"][0]) & 0xFFFFFFFFFFFFFFFF for r in rows])
            rrows_h = (C.c_int32 * n)(*[int(r["key"][1]) for r in rows])
            rs_h = row_sampling_array([r["sampling"] for r in rows]) if self.per_row else None
            if limits is not None:
                _lib.check(l.gsv_t2s_set_row_limits(dec._h, row_limits_array(limits), n), "gsv_t2s_set_row_limits")
            _lib.check(l.gsv_t2s_session_admit(dec._h, n, C.cast(slots_h, C.c_void_p), phones.data_ptr(), C.cast(lens_h, C.c_void_p),
                                               bert_dev.data_ptr() if bert_dev is not None else None,
                                               pr.data_ptr() if pr.numel() else None,
                                               C.cast(plens_h, C.c_void_p), C.cast(seeds_h, C.c_void_p), C.cast(rrows_h, C.c_void_p),
                                               C.cast(rs_h, C.c_void_p) if rs_h is not None else None,
                                               C.c_void_p(dec.stream.cuda_stream)), "gsv_t2s_session_admit")
            torch.cuda.current_stream(dev).wait_stream(dec.stream)
            ms, nb = C.c_float(0), C.c_int64(0)
            _lib.check(l.gsv_t2s_session_adopt_info(dec._h, C.byref(ms), C.byref(nb)), "gsv_t2s_session_adopt_info")
            self.adopt.append((n, ms.value, nb.value))
        tickets = []
        for s, p_, b_ in zip(slots, prompts, budgets):
            self._row_budget[s] = b_
            self._owner[s] = self._next_ticket
            self._prompt[s] = p_.to(dev, torch.int64)
            tickets.append(self._next_ticket)
            self.history.append((self._next_ticket, s))
            self._next_ticket += 1
        return tickets

    def release(self, tickets: Sequence[int]) -> List[int]:
        """takes the rows of these tickets out of the session (gsv_t2s_session_release): no advance reports them, and their
        slots are free for the next admission.  A ticket that holds no slot (finished and reported, or never admitted) is
        skipped.  Returns the slots that were released."""
        wanted = set(int(t) for t in tickets)
        slots = [s for s in range(self.slots) if self._owner[s] is not None and self._owner[s] in wanted]
        return self.release_slots(slots)

    def release_slots(self, slots: Sequence[int]) -> List[int]:
        """`release` by slot number, unchecked on this side: the engine refuses a slot out of range or given twice"""
        slots = [int(s) for s in slots]
        if not slots:
            return []
        dev, n = self.dec.device, len(slots)
        with torch.cuda.device(dev):
            self.dec.stream.wait_stream(torch.cuda.current_stream(dev))
            slots_h = (C.c_int32 * n)(*slots)
            _lib.check(_lib.lib().gsv_t2s_session_release(self.dec._h, n, C.cast(slots_h, C.c_void_p),
                                                          C.c_void_p(self.dec.stream.cuda_stream)), "gsv_t2s_session_release")
            torch.cuda.current_stream(dev).wait_stream(self.dec.stream)
        for s in slots:
            self._owner[s], self._prompt[s] = None, None
        return slots

    def state(self) -> np.ndarray:
        """test hook: int32 [4][slots] = cached positions | live | step counter | prompt length of every slot"""
        st = np.zeros((4, self.slots), dtype=np.int32)
        _lib.check(_lib.lib().gsv_t2s_session_state(self.dec._h, st.ctypes.data), "gsv_t2s_session_state")
        return st

    def advance(self, steps: int):
        """at most `steps` further steps for every live row; returns [(ticket, y, idx)] of the rows that have finished, y = prompt +
        generated tokens and idx = their count, as `Text2SemanticDecoder._run` returns them.  Their slots are free again."""
        dec, dev = self.dec, self.dec.device
        l = _lib.lib()
        live_h, steps_h = (C.c_int * self.slots)(), (C.c_int * self.slots)()
        with torch.cuda.device(dev):
            dec.stream.wait_stream(torch.cuda.current_stream(dev))
            _lib.check(l.gsv_t2s_session_advance(dec._h, int(steps), live_h, steps_h, C.c_void_p(dec.stream.cuda_stream)),
                       "gsv_t2s_session_advance")
            torch.cuda.current_stream(dev).wait_stream(dec.stream)
            mode, _, ran = dec.decode_info()
            if ran or mode:
                self.modes.append(mode)
            done = [s for s in range(self.slots) if self._owner[s] is not None and not live_h[s]]
            out = []
            if done:
                idx = self.out_len.cpu().tolist()
                for s in done:
                    n = idx[s]
                    out.append((self._owner[s], torch.cat([self._prompt[s], self.out_tokens[s, :n].long()]), n))
                    if self.dump is not None:
                        self.logits[self._owner[s]] = self.dump[:steps_h[s], s].clone()
                    if self.logp is not None:
                        self.logprobs[self._owner[s]] = self.logp[s, :n + 1].clone()
                        self.cut[self._owner[s]] = n >= self._row_budget[s] - 1
                    self._owner[s], self._prompt[s] = None, None
        return out


class Text2SemanticDecoder:
    def __init__(self, config: dict, device="cuda:0", dtype=torch.float16, max_batch: int = 32,
                 max_seq: int = 2048, norm_first: bool = False, top_k: int = 3):
        m = config["model"]
        self.config = config
        self.model_dim = m["hidden_dim"]
        self.embedding_dim = m["embedding_dim"]
        self.num_head = m["head"]
        self.num_layers = m["n_layer"]
        self.vocab_size = m["vocab_size"]
        self.phoneme_vocab_size = m["phoneme_vocab_size"]
        self.EOS = m["EOS"]
        assert self.EOS == self.vocab_size - 1
        assert not norm_first, "the reference's inference checkpoints are post-LN"
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("gsv Text2SemanticDecoder runs on an MI355X (cuda/HIP device) only; "
                               "there is no CPU path in the product")
        self.dtype = dtype
        self.max_batch = max_batch
        self.max_seq = max_seq
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        with torch.cuda.device(self.device):
            _lib.init(idx)
            cfg = _lib.T2SConfig(self.num_layers, self.model_dim, self.num_head, 4 * self.model_dim,
                                 self.vocab_size, self.phoneme_vocab_size, 1024)
            h = C.c_void_p()
            _lib.check(_lib.lib().gsv_t2s_create(C.byref(cfg), _lib.dtype_code(dtype), max_batch, max_seq,
                                                 C.byref(h)), "gsv_t2s_create")
            self._h = h
            self.stream = torch.cuda.Stream(device=self.device)
        self._loaded = False
        self.infer_panel = self.infer_panel_naive

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                _lib.lib().gsv_t2s_destroy(h)
            except Exception:
                pass
            self._h = None

    # ---- weights -------------------------------------------------------------------
    def load_state_dict(self, state_dict: Dict[str, torch.Tensor], strict: bool = True):
        """Accepts the reference checkpoint's `weight` dict (keys with or without the
        Lightning `model.` prefix, reference TTS_infer_pack/TTS.py:590-603)."""
        if self._loaded:
            raise RuntimeError("weights already loaded; create a new Text2SemanticDecoder")
        l = _lib.lib()
        with torch.cuda.device(self.device):
            _lib.load_tensors(l.gsv_t2s_load_tensor, self._h, ((k, v) for k, v in state_dict.items() if torch.is_tensor(v)))
            _lib.load_tensors(l.gsv_t2s_load_tensor, self._h, [("pe", _sine_pe(4000, self.embedding_dim))])
            _lib.check(l.gsv_t2s_finalize(self._h), "gsv_t2s_finalize")
        self._loaded = True
        return self

    # ---- engine call ---------------------------------------------------------------
    def _bert_rows(self, bert, lens):
        """the rows' BERT features [1024, X_b] as one device tensor [sum(X_b), 1024], or None where they are all zero"""
        dev = self.device
        bert_dev = None
        if bert is not None and any(b_ is not None for b_ in bert):
            # None or all-zero features (non-zh text): bert_proj(0) is its bias, handled in the engine.  Host tensors are
            # tested on the host and travel as ONE copy (the pipeline hands over 32 zero blocks of 330 KB per batch: as 32
            # pageable uploads + a device-side any() + sync they were ~1 ms of idle GPU in front of every prefill)
            on_host = all(b_ is None or b_.device.type == "cpu" for b_ in bert)
            if on_host:
                # numpy on the host view: a torch reduction costs ~1.3 ms per block on a many-core host (thread wake-up), i.e.
                # 40 ms per batch of 32 (tools/prefill_probe.py)
                if any(b_ is not None and _host_nonzero(b_) for b_ in bert):
                    cols = [(torch.zeros(lens[i], 1024) if b_ is None else b_.reshape(1024, -1).t().float())
                            for i, b_ in enumerate(bert)]
                    bert_dev = torch.cat(cols, 0).contiguous().to(dev)
            else:
                cols = [(torch.zeros(lens[i], 1024, device=dev) if b_ is None
                         else b_.reshape(1024, -1).t().to(dev, torch.float32)) for i, b_ in enumerate(bert)]
                allb = torch.cat(cols, 0).contiguous()
                if bool(torch.any(allb)):            # one host sync for the whole batch
                    bert_dev = allb
        return bert_dev

    def _run(self, x: Sequence[torch.Tensor], prompts: torch.Tensor, bert: Sequence[torch.Tensor], top_k, top_p,
             early_stop_num, temperature, repetition_penalty, eos_mask_steps, noise=None, seed=0,
             max_steps: int = 1500, force_tokens=None, dump_logits=False, rng_keys=None, row_sampling=None, logprobs=False,
             row_limits=None):
        """prompts: [B, P] (one prompt length for the batch; P = 0 or None: prompt-free) or a list of B 1-D prompts of
        lengths P_b >= 1 (ragged: gsv_t2s_prefill_ragged).  rng_keys: optional [(seed_b, row_b)] per row, the counter-RNG
        key that replaces (seed, b) (gsv_t2s_set_row_rng; row_b in [0, 2**24), anything else is refused).  row_sampling: optional [(top_k, top_p, temperature,
        repetition_penalty)] per row, which replace the four scalar arguments for this call (gsv_t2s_set_row_sampling).
        logprobs=True leaves last_logprobs: B 1-D fp32 tensors, row b's idx[b] + 1 log-probabilities of the tokens it took
        under the model's own distribution (gsv_t2s_set_logprobs): the generated tokens, then the finishing step; and
        last_cut: per row, whether the step budget ended it instead of EOS.  row_limits: optional [(eos_mask_steps,
        early_stop_num, max_steps)] per row, which replace eos_mask_steps, early_stop_num and max_steps for this call
        (gsv_t2s_set_row_limits); every row is then held to its own budget, the K/V arena's bound included, and a list of
        prompts may hold None or empty prompts: prompt-free rows."""
        if not self._loaded:
            raise RuntimeError("load_state_dict() first")
        B = len(x)
        if row_sampling is not None and len(row_sampling) != B:
            raise ValueError(f"{len(row_sampling)} sampling tuples for {B} rows")
        if row_limits is not None and len(row_limits) != B:
            raise ValueError(f"{len(row_limits)} limit tuples for {B} rows")
        dev = self.device
        if prompts is None:                  # prompt-free (reference t2s_model.py:849-856): empty audio prefix
            prompts = torch.zeros(B, 0, dtype=torch.int64)
        ragged = isinstance(prompts, (list, tuple))
        if ragged:
            if len(prompts) != B:
                raise ValueError(f"{len(prompts)} prompts for {B} rows")
            prompts = [torch.zeros(0, dtype=torch.int64) if p_ is None else p_ for p_ in prompts]
            plens = [int(p_.reshape(-1).shape[0]) for p_ in prompts]
            if min(plens) < 1 and row_limits is None:
                raise ValueError("ragged prompts must each hold at least one token (prompt-free rows: prompts=None)")
        if rng_keys is not None and len(rng_keys) != B:
            raise ValueError(f"{len(rng_keys)} RNG keys for {B} rows")
        l = _lib.lib()
        with torch.cuda.device(dev):
            lens = [int(t.shape[-1]) for t in x]
            if ragged:
                P = max(plens)
                need = max(n_ + p_ for n_, p_ in zip(lens, plens)) + 2
            else:
                P = int(prompts.shape[1])
                need = max(lens) + P + 2
            wanted = max_steps if early_stop_num in (-1, None) else min(max_steps, int(early_stop_num) + 1)
            budget = min(wanted, self.max_seq - need)
            limits = None
            if row_limits is not None:
                needs = [n_ + (p_ if ragged else P) + 2 for n_, p_ in zip(lens, plens if ragged else lens)]
                limits, budgets, short = row_limit_tuples(row_limits, needs, self.max_seq)
                need = needs[budgets.index(min(budgets))]
                budget = max(budgets) if min(budgets) >= 1 else 0
            if budget < 1:
                raise ValueError(f"sequence of {need} positions does not fit max_seq={self.max_seq}")
            arena_bound = budget < wanted if limits is None else short
            phones = torch.cat([t.reshape(-1) for t in x]).to(dev, torch.int32).contiguous()
            lens_h = (C.c_int32 * B)(*lens)
            bert_dev = self._bert_rows(bert, lens)
            if ragged:
                pr = torch.cat([p_.reshape(-1).to(dev, torch.int32) for p_ in prompts]).contiguous()
            else:
                pr = prompts.to(dev, torch.int32).contiguous()
            out_tokens = torch.zeros(B, budget, dtype=torch.int32, device=dev)
            out_len = torch.full((B,), -1, dtype=torch.int32, device=dev)
            logp = torch.full((B, budget), float("nan"), dtype=torch.float32, device=dev) if logprobs else None
            noise_dev, noise_rows = None, 0
            if noise is not None:
                noise_dev = noise.to(dev, torch.float32).contiguous()
                assert noise_dev.dim() == 3 and noise_dev.shape[2] == self.vocab_size and noise_dev.shape[0] >= budget
                noise_rows = noise_dev.shape[1]
                noise_dev = noise_dev[:budget].contiguous()
            self.stream.wait_stream(torch.cuda.current_stream(dev))
            sp = _lib.SamplingParams(int(top_k) if top_k is not None else 0, float(top_p if top_p is not None else 1.0),
                                     float(temperature), float(repetition_penalty),
                                     -1 if early_stop_num is None else int(early_stop_num), int(eos_mask_steps),
                                     int(budget), int(seed) & 0xFFFFFFFFFFFFFFFF)
            if early_stop_num not in (-1, None) and budget < int(early_stop_num) + 1:
                sp.early_stop_num = -1   # the arena bound (max_steps) ends generation first
            s = C.c_void_p(self.stream.cuda_stream)
            if limits is not None:   # in front of the prefill: they are what lets it take prompt-free rows
                _lib.check(l.gsv_t2s_set_row_limits(self._h, row_limits_array(limits), B), "gsv_t2s_set_row_limits")
            if ragged:
                plens_h = (C.c_int32 * B)(*plens)
                _lib.check(l.gsv_t2s_prefill_ragged(self._h, phones.data_ptr(), C.cast(lens_h, C.c_void_p), B,
                                                    bert_dev.data_ptr() if bert_dev is not None else None,
                                                    pr.data_ptr() if pr.numel() else None, C.cast(plens_h, C.c_void_p), s),
                           "gsv_t2s_prefill_ragged")
            else:
                _lib.check(l.gsv_t2s_prefill(self._h, phones.data_ptr(), C.cast(lens_h, C.c_void_p), B,
                                             bert_dev.data_ptr() if bert_dev is not None else None,
                                             pr.data_ptr() if P > 0 else None, P, s),
                           "gsv_t2s_prefill")
            # the prefill's last conv / GEMM launch (FFN2 of the last layer): which kernel family served it (include/gsv.h)
            self.last_prefill_route = int(l.gsv_debug_last_conv_route(0))
            if rng_keys is not None:
                seeds_h = (C.c_uint64 * B)(*[int(k[0]) & 0xFFFFFFFFFFFFFFFF for k in rng_keys])
                rows_h = (C.c_int32 * B)(*[int(k[1]) for k in rng_keys])
                _lib.check(l.gsv_t2s_set_row_rng(self._h, C.cast(seeds_h, C.c_void_p), C.cast(rows_h, C.c_void_p), B),
                           "gsv_t2s_set_row_rng")
            if row_sampling is not None:
                _lib.check(l.gsv_t2s_set_row_sampling(self._h, row_sampling_array(row_sampling), B), "gsv_t2s_set_row_sampling")
            steps = C.c_int(0)
            dump = None
            if force_tokens is not None or dump_logits:
                # parity hooks (tests): teacher forcing and the per-step logits of whichever decode path runs
                ft = None
                if force_tokens is not None:
                    ft = torch.zeros(B, budget, dtype=torch.int32, device=dev)
                    src = force_tokens.to(dev, torch.int32)
                    n = min(budget, int(src.shape[1]))
                    ft[:, :n] = src[:, :n]
                drawn = None
                if dump_logits:
                    dump = torch.zeros(budget, B, self.vocab_size, dtype=torch.float32, device=dev)
                    drawn = torch.full((budget, B, 2), -1, dtype=torch.int32, device=dev)
                torch.cuda.current_stream(dev).synchronize()
                _lib.check(l.gsv_t2s_set_debug(self._h, ft.data_ptr() if ft is not None else None,
                                               dump.data_ptr() if dump is not None else None,
                                               drawn.data_ptr() if drawn is not None else None), "gsv_t2s_set_debug")
                self.last_drawn_dump = drawn
            self.last_logits_dump = dump
            if logp is not None:
                _lib.check(l.gsv_t2s_set_logprobs(self._h, logp.data_ptr()), "gsv_t2s_set_logprobs")
            _lib.check(l.gsv_t2s_decode(self._h, C.byref(sp), noise_dev.data_ptr() if noise_dev is not None else None,
                                        noise_rows, out_tokens.data_ptr(), out_len.data_ptr(), C.byref(steps), s),
                       "gsv_t2s_decode")
            torch.cuda.current_stream(dev).wait_stream(self.stream)
            idx = out_len.cpu().tolist()
            self.last_steps = steps.value
            if ragged:
                y_all = None
                offs = np.concatenate([[0], np.cumsum(plens)]).tolist()
                gen_all = out_tokens.long()
                pr_all = pr.long()
            else:
                y_all = torch.cat([pr, out_tokens], dim=1).long()       # one concat for the batch; rows are sliced as views
            y_list = []
            self.last_truncated = [b for b in range(B) if idx[b] < 0] if arena_bound else []
            if self.last_truncated:
                # the reference always allows 1500 steps (t2s_model.py:694) or early_stop_num; here the K/V arena ended
                # these rows first -- never silently
                warnings.warn(f"Text2SemanticDecoder: rows {self.last_truncated} were cut after {steps.value - 1} tokens by the "
                              f"K/V arena (max_seq={self.max_seq}, {need} positions used by text + prompt); create the "
                              f"decoder with a larger max_seq", RuntimeWarning, stacklevel=3)
            for b in range(B):
                n = idx[b] if idx[b] >= 0 else steps.value - 1
                idx[b] = n
                if ragged:
                    y_list.append(torch.cat([pr_all[offs[b]:offs[b + 1]], gen_all[b, :n]]))
                else:
                    y_list.append(y_all[b, :P + n])
            self.last_logprob_buffer = logp     # [B][budget], NaN where a row ran no step; last_logprobs are views of it
            self.last_logprobs = None if logp is None else [logp[b, :idx[b] + 1] for b in range(B)]
            self.last_cut = None if logp is None else [idx[b] >= (budget if limits is None else budgets[b]) - 1 for b in range(B)]
        return y_list, idx

    # ---- reference entry points -----------------------------------------------------
    @torch.no_grad()
    def infer_panel_batch_infer(self, x: List[torch.LongTensor], x_lens: torch.LongTensor, prompts: torch.LongTensor,
                                bert_feature: List[torch.Tensor], top_k: int = -100, top_p: int = 100,
                                early_stop_num: int = -1, temperature: float = 1.0,
                                repetition_penalty: float = 1.35, **kwargs):
        """reference t2s_model.py:583-779: returns (y_list, idx_list); y_list[i] = prompt + generated
        tokens (finishing token dropped), idx_list[i] = number of generated tokens.

        `prompts` is the reference's [B, P] tensor, or a list of B 1-D prompts of different lengths (one reference voice
        per row, every length >= 1).  kwarg `rng_keys=[(seed, row), ...]`: row i draws with the counter-RNG key
        (seed, row) instead of (seed kwarg, its row in the launch), so it samples the same tokens whichever batch it
        is decoded in.  kwarg `row_sampling=[(top_k, top_p, temperature, repetition_penalty), ...]`: row i samples with
        its own tuple instead of the four arguments (parallel decode only; the prompt-free loop takes the arguments).
        kwarg `logprobs=True`: last_logprobs / last_cut of `_run`, for all rows in input order (parallel decode only)."""
        rng_keys = kwargs.get("rng_keys")
        if rng_keys is not None and len(rng_keys) != len(x):
            raise ValueError(f"{len(rng_keys)} RNG keys for {len(x)} rows")
        row_sampling = kwargs.get("row_sampling")
        if row_sampling is not None and len(row_sampling) != len(x):
            raise ValueError(f"{len(row_sampling)} sampling tuples for {len(x)} rows")
        if prompts is None:
            return self.infer_panel_naive_batched(x, x_lens, prompts, bert_feature, top_k=top_k, top_p=top_p,
                                                  early_stop_num=early_stop_num, temperature=temperature, **kwargs)
        out = []
        ys: List[Optional[torch.Tensor]] = [None] * len(x)
        idxs: List[Optional[int]] = [None] * len(x)
        want_lp = bool(kwargs.get("logprobs", False))
        lps, cuts = [], []
        noise = kwargs.get("noise")
        for lo in range(0, len(x), self.max_batch):
            hi = min(lo + self.max_batch, len(x))
            nz = noise
            if noise is not None and noise.shape[1] > 1:
                nz = noise[:, lo:hi]
            y, i = self._run(x[lo:hi], prompts[lo:hi], bert_feature[lo:hi], top_k, top_p, early_stop_num, temperature,
                             repetition_penalty, eos_mask_steps=1, noise=nz, seed=kwargs.get("seed", 0),
                             max_steps=kwargs.get("max_steps", 1500),
                             force_tokens=None if kwargs.get("force_tokens") is None else kwargs["force_tokens"][lo:hi],
                             dump_logits=kwargs.get("dump_logits", False),
                             rng_keys=None if rng_keys is None else list(rng_keys[lo:hi]),
                             row_sampling=None if row_sampling is None else list(row_sampling[lo:hi]), logprobs=want_lp)
            ys[lo:hi] = y
            idxs[lo:hi] = i
            if want_lp:
                lps += self.last_logprobs
                cuts += self.last_cut
        self.last_logprobs, self.last_cut = (lps, cuts) if want_lp else (None, None)
        return ys, idxs

    # ---- decode sessions: continuous batching ------------------------------------------
    def open_session(self, slots: int, top_k, top_p, temperature, repetition_penalty, early_stop_num, eos_mask_steps: int = 1,
                     max_steps: int = 1500, row_sampling: bool = False, row_limits: bool = False, **debug) -> T2SSession:
        """Opens a decode session of `slots` rows (<= max_batch); until it is closed the other entry points of this decoder
        raise.  The four sampling values hold for every row unless row_sampling=True, in which case each admitted row brings
        its own tuple.  debug: force=True / dump_logits=True, the parity hooks of `_run`, per slot.  logprobs=True: the
        session fills `logprobs[ticket]` / `cut[ticket]` (what `_run(logprobs=True)` leaves for a row) when `advance` reports
        the row.  row_limits=True: admitted rows may bring limits=(eos_mask_steps, early_stop_num, max_steps) of their own, none
        above this session's budget, and prompt=None (T2SSession.admit)."""
        return T2SSession(self, slots, top_k, top_p, temperature, repetition_penalty, early_stop_num, eos_mask_steps, max_steps,
                          row_sampling=row_sampling, row_limits=row_limits, **debug)

    @torch.no_grad()
    def infer_panel_continuous(self, x: List[torch.LongTensor], prompts, bert_feature: List[torch.Tensor], top_k: int = -100,
                               top_p: int = 100, early_stop_num: int = -1, temperature: float = 1.0,
                               repetition_penalty: float = 1.35, rng_keys=None, row_sampling=None, slots: Optional[int] = None,
                               chunk: int = 32, admit_min: Optional[int] = None, max_steps: int = 1500, force_tokens=None,
                               dump_logits: bool = False, logprobs: bool = False, row_limits=None):
        """`infer_panel_batch_infer` for a queue of any length through ONE decode session: rows are admitted in the order given
        whenever `admit_min` slots are free (default max(1, slots // 4); see admit_count), `chunk` steps run between admissions
        (both defaults from the sweep of tools/continuous_ar_bench.py, profiles/continuous_ar.txt),
        and a row that has finished hands its slot to the next row of the queue while its neighbours go on decoding.  Returns
        (ys, idx) in input order.  rng_keys=[(seed, row)] is required: a row's draws must not depend on where and when it is
        decoded.  A row whose text + prompt leave the K/V arena less than the full step budget is decoded on its own by the
        ordinary path after the session (and listed in last_truncated if the arena cuts it), as it would be there.
        force_tokens [N][steps] / dump_logits: the parity hooks of `_run` (tests); last_logits_dump is then a list of N
        [steps run][vocab] tensors.  logprobs=True: last_logprobs / last_cut of `_run`, in input order.  last_session is the
        closed session (its history, modes and adopt times).  row_limits=True: a row short of arena room is admitted with its
        smaller budget instead; row_limits=[(eos_mask_steps, early_stop_num, max_steps) | None, ...]: the rows' own limits
        as well (none above this call's budget), and prompts[i] may be None: a prompt-free row."""
        N = len(x)
        per_limits = row_limits if isinstance(row_limits, (list, tuple)) else None
        if per_limits is not None and len(per_limits) != N:
            raise ValueError(f"{len(per_limits)} limit tuples for {N} rows")
        if rng_keys is None or len(rng_keys) != N:
            raise ValueError("infer_panel_continuous needs one RNG key (seed, row) per row")
        if row_sampling is not None and len(row_sampling) != N:
            raise ValueError(f"{len(row_sampling)} sampling tuples for {N} rows")
        if prompts is None:
            raise ValueError("prompt-free rows are decoded by infer_panel_batch_infer (the naive loop)")
        slots = self.max_batch if slots is None else int(slots)
        admit_min = max(1, slots // 4) if admit_min is None else int(admit_min)
        wanted = max_steps if early_stop_num in (-1, None) else min(max_steps, int(early_stop_num) + 1)
        rows = [dict(x=x[i], bert=bert_feature[i] if bert_feature is not None else None,
                     prompt=torch.zeros(0, dtype=torch.int64) if prompts[i] is None else prompts[i].reshape(-1),
                     key=rng_keys[i], sampling=None if row_sampling is None else row_sampling[i]) for i in range(N)]
        es = -1 if early_stop_num is None else int(early_stop_num)
        for i, r in enumerate(rows):
            if per_limits is not None and per_limits[i] is not None:
                r["limits"] = tuple(per_limits[i])
            elif row_limits and int(r["x"].shape[-1]) + int(r["prompt"].shape[0]) + 2 + wanted > self.max_seq:
                r["limits"] = (1, es, int(max_steps))       # the session's scalars: admit() bounds the budget by the arena
        if force_tokens is not None:
            for i, r in enumerate(rows):
                r["force"] = force_tokens[i]
        fits = [bool(row_limits) or int(r["x"].shape[-1]) + int(r["prompt"].shape[0]) + 2 + wanted <= self.max_seq for r in rows]
        if (force_tokens is not None or dump_logits) and not all(fits):
            raise ValueError("the parity hooks need every row to fit the K/V arena with its full budget")
        queue = [i for i in range(N) if fits[i]]
        ys: List[Optional[torch.Tensor]] = [None] * N
        idxs: List[Optional[int]] = [None] * N
        lps: List[Optional[torch.Tensor]] = [None] * N
        cuts: List[Optional[bool]] = [None] * N
        if queue:
            with self.open_session(slots, top_k, top_p, temperature, repetition_penalty, early_stop_num, 1, max_steps,
                                   row_sampling=row_sampling is not None, force=force_tokens is not None,
                                   dump_logits=dump_logits, logprobs=logprobs, row_limits=bool(row_limits)) as ses:
                q, where = 0, {}
                while q < len(queue) or ses.live:
                    k = admit_count(len(ses.free), len(queue) - q, ses.live, admit_min)
                    if k:
                        for t, i in zip(ses.admit([rows[i] for i in queue[q:q + k]]), queue[q:q + k]):
                            where[t] = i
                        q += k
                    for t, y, n in ses.advance(chunk):
                        ys[where[t]], idxs[where[t]] = y, n
                self.last_session = ses
                if dump_logits:
                    by_row = {i: ses.logits[t] for t, i in where.items()}
                    self.last_logits_dump = [by_row[i] for i in range(N)]
                if logprobs:
                    for t, i in where.items():
                        lps[i], cuts[i] = ses.logprobs[t], ses.cut[t]
        truncated = []
        for i in range(N):
            if fits[i]:
                continue
            r = rows[i]
            sk = (top_k, top_p, temperature, repetition_penalty) if r["sampling"] is None else r["sampling"]
            y, n = self._run([r["x"]], [r["prompt"]], [r["bert"]], sk[0], sk[1], early_stop_num, sk[2], sk[3], eos_mask_steps=1,
                             max_steps=max_steps, rng_keys=[r["key"]], logprobs=logprobs)
            ys[i], idxs[i] = y[0], n[0]
            if logprobs:
                lps[i], cuts[i] = self.last_logprobs[0], self.last_cut[0]
            truncated += [i] * bool(self.last_truncated)
        self.last_truncated = truncated
        self.last_logprobs, self.last_cut = (lps, cuts) if logprobs else (None, None)
        return ys, idxs

    @torch.no_grad()
    def infer_panel_naive(self, x: torch.LongTensor, x_lens: torch.LongTensor, prompts: torch.LongTensor,
                          bert_feature: torch.Tensor, top_k: int = -100, top_p: int = 100, early_stop_num: int = -1,
                          temperature: float = 1.0, repetition_penalty: float = 1.35, **kwargs):
        """reference t2s_model.py:814-918: batch 1, EOS masked while idx < 11; returns (y[:, :-1], idx)."""
        y, i = self._run([x[0]], prompts, [bert_feature[0] if bert_feature is not None else None], top_k, top_p, early_stop_num, temperature,
                         repetition_penalty, eos_mask_steps=11, noise=kwargs.get("noise"), seed=kwargs.get("seed", 0),
                         max_steps=kwargs.get("max_steps", 1500))
        return y[0].unsqueeze(0), (0 if prompts is None else i[0])      # prompt-free reports idx 0 (t2s_model.py:916-917)

    @torch.no_grad()
    def infer_panel_naive_batched(self, x, x_lens, prompts, bert_feature, top_k: int = -100, top_p: int = 100,
                                  early_stop_num: int = -1, temperature: float = 1.0,
                                  repetition_penalty: float = 1.35, **kwargs):
        """reference t2s_model.py:781-812: the naive loop per item."""
        y_list, idx_list = [], []
        for i in range(len(x)):
            y, idx = self.infer_panel_naive(x[i].unsqueeze(0), x_lens[i] if x_lens is not None else None,
                                            prompts[i].unsqueeze(0) if prompts is not None else None,
                                            [bert_feature[i]] if bert_feature[i] is None else bert_feature[i].unsqueeze(0),
                                            top_k, top_p, early_stop_num, temperature,
                                            repetition_penalty, **kwargs)
            y_list.append(y[0])
            idx_list.append(idx)
        return y_list, idx_list

    # ---- decode-engine selection / report -------------------------------------------
    def set_mega(self, on: bool):
        """A/B switch: False makes later calls use the launch-per-phase decode step instead of the persistent engine
        (csrc/t2s_mega.hip; fp16, v1/v2 shape, batch <= 128 in one launch)."""
        _lib.check(_lib.lib().gsv_t2s_set_mega(self._h, int(bool(on))), "gsv_t2s_set_mega")

    def set_prefill_gemm(self, mode: int):
        """A/B switch of the prefill's per-layer GEMMs: 0 = the dispatcher only, 1 = the panel kernel (csrc/gemm_panel.hip)
        wherever it is eligible, 2 (default) = the panel kernel from the measured row-count threshold upwards.  Same bits
        either way; GSV_NO_PREFILL_PANEL in the environment forces 0."""
        _lib.check(_lib.lib().gsv_t2s_set_prefill_gemm(self._h, int(mode)), "gsv_t2s_set_prefill_gemm")

    def debug_kv(self, layer: int, which: int, row: int, n_pos: int):
        """test hook: cached positions 0 .. n_pos - 1 of batch row `row` in one layer's K (which = 0) or V (1): [heads][n_pos][32]"""
        out = torch.empty(self.num_head, n_pos, 32, dtype=self.dtype)
        _lib.check(_lib.lib().gsv_t2s_debug_kv(self._h, layer, which, row, n_pos, out.data_ptr()), "gsv_t2s_debug_kv")
        return out

    def debug_stall(self, member: int):
        """test hook: the next persistent launch loses one hand-off publish of `member` (group 0)"""
        _lib.check(_lib.lib().gsv_t2s_debug_stall(self._h, int(member)), "gsv_t2s_debug_stall")

    def engine_stats(self):
        """(engine_available, fallbacks, (epoch, workgroup, hop code) of the last hand-off timeout): a persistent launch
        that times out is re-run on the launch-per-phase step and the handle stops using the engine."""
        av, fb, e3 = C.c_int(0), C.c_int(0), (C.c_uint * 3)()
        _lib.check(_lib.lib().gsv_t2s_engine_stats(self._h, C.byref(av), C.byref(fb), e3), "gsv_t2s_engine_stats")
        return bool(av.value), fb.value, tuple(e3)

    def decode_info(self):
        """(mode, device_ms, steps) of the last decode call: mode 1 = persistent engine, 0 = launch per phase."""
        mode, ms, steps = C.c_int(0), C.c_float(0), C.c_int(0)
        _lib.check(_lib.lib().gsv_t2s_decode_info(self._h, C.byref(mode), C.byref(ms), C.byref(steps)), "gsv_t2s_decode_info")
        return mode.value, ms.value, steps.value

    # ---- measurement hooks (bench.py) ----------------------------------------------
    def debug_logits(self, B: int) -> torch.Tensor:
        out = torch.empty(B, self.vocab_size, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().gsv_t2s_debug_logits(self._h, out.data_ptr(), C.c_void_p(self.stream.cuda_stream)))
            self.stream.synchronize()
        return out

    def time_attention(self, iters: int = 20):
        """(avg ms per decode-attention launch, algorithmic HBM bytes per launch, algorithmic bytes of a
        whole decode step, eager ms of one step's 24-layer kernel sequence) at the current cache state,
        measured in situ with HIP events on the engine stream (gsv_t2s_time_step)."""
        ms = C.c_float(0)
        step = C.c_float(0)
        ab = C.c_int64(0)
        with torch.cuda.device(self.device):
            l = _lib.lib()
            _lib.check(l.gsv_t2s_time_step(self._h, iters, C.byref(step), C.byref(ms), C.c_void_p(self.stream.cuda_stream)))
            total = l.gsv_t2s_step_bytes(self._h, C.byref(ab))
        return ms.value, ab.value, total, step.value
