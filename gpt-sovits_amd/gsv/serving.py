"""Serving requests as they arrive: one open AR decode session, shared waveform passes.

`TTS.run_batch` takes a closed list and returns when the slowest request is done.  Here requests come in one by one:

* `Scheduler` is the core, single-threaded and deterministic.  `submit` only enqueues; every `step` takes in what was submitted,
  admits queued sentences into the free slots of ONE decode session (`T2SSession`, per-row keys and sampling values), advances
  the live rows a chunk of steps, and sends the requests whose sentences have all come back through the shared waveform stage
  of `run_batch` -- so a short request is delivered when it is finished, and a new one takes a free slot while the others
  decode.  A request that cannot decode in the session (prompt-free, `parallel_infer=False`, a row the K/V arena would cut,
  `best_of` candidates) is *exclusive*: a FIFO barrier that is served with `run_batch([request])` once nothing is live.
* A streaming request (`return_fragment` / `streaming_mode`) is a session citizen like any other, delivered fold by fold: a fold
  (one `to_batch` batch, what `run()` yields a fragment for) whose sentences are all back goes into that step's waveform pass
  at once -- or, `continuous_cfm`, its rows join the flow-matching FIFO at once -- and its fragment is emitted as soon as its
  audio exists and every earlier fold of the request has been emitted.  All fragments of a step are converted by one
  `gsv_postprocess_groups` launch pair and one copy (`TTS.postprocess_fragments`).  `Scheduler.take_fragments()` hands out the
  fragments of the last step, `Server.submit_stream` an iterator over one request's; the request's result is the list of all.
* `plan_online` is the schedule as a pure function, `plan_continuous` with arrivals: the event trace `Scheduler` records in
  `stats["events"]`.  The two share the policies -- `_Policy` and `_CfmPolicy` hold every decision and touch no GPU -- and the
  step itself: `_run_step` is the one place that asks the policies in order, appends the events and, for everything that is
  not a decision, calls a backend.  `plan_online`'s backend is `_Replay`, which counts the `lengths` down and looks the
  flow-matching rows up in `cfm_folds`; `Scheduler` is its own backend and makes the GPU calls.
* `Server` puts one loop thread around a scheduler: the only thread that makes GPU calls.  `submit` returns a
  `concurrent.futures.Future` from any thread.
* `Scheduler(continuous_cfm=True)` (v3 / v4) keeps a second session open behind the first: a flow-matching session
  (`CFMSession`) whose rows carry their own step count, guidance rate and LoRA slot.  A request whose sentences are back is
  encoded at once and its rows queue for the session's slots; a scheduler step runs at most `cfm_chunk` Euler steps, fetches
  the rows that finished with one `fetch_mel` launch -- de-normalised and channels-first, the vocoder's input as it stands --
  vocodes the folds that are complete and delivers the requests that are.  `_CfmPolicy` holds these decisions next to
  `_Policy`, and `plan_online(cfm_folds=...)` runs the same step over them.  An exclusive request waits for both sessions and
  closes both.  AR launches, Euler steps and vocoder calls still run strictly one after the other, on the one thread.

What a request returns is what `run_batch([request])` returns for it alone: its rows carry the RNG keys and sampling tuples
`plan_batch` gives them, sampling is per row, admissions and releases leave the neighbouring slots untouched, and the waveform
stages are the ones `run_batch` pins against `run`.  AR launches and waveform passes are issued strictly one after the other
(DESIGN.md section 4o).
"""
from __future__ import annotations

import collections
import concurrent.futures
import queue
import threading
from concurrent.futures import CancelledError
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

from .AR.models.t2s_model import admit_count


class _Stream:
    """What `_Policy` knows of a streaming request, which is delivered fragment by fragment, one fragment per fold."""
    __slots__ = ("fold", "missing", "voiced", "nxt", "n")

    def __init__(self, folds: Sequence[int]):
        self.fold = [bi for bi, n in enumerate(folds) for _ in range(n)]       # the fold of each row, rows being in fold order
        self.missing = {bi: int(n) for bi, n in enumerate(folds)}              # fold -> rows not back yet
        self.voiced: set = set()                   # the folds whose audio exists and that wait for an earlier one
        self.nxt, self.n = 0, len(folds)           # the next fold to emit; its folds

    def __getitem__(self, field: str):             # st["fold"] is st.fold: the state still reads by key, as a dict did
        return getattr(self, field)


class _Policy:
    """Every scheduling decision of `Scheduler` and `plan_online`, as host-only state: the FIFO of requests whose rows wait,
    the row in each slot, the rows each request still misses, and the requests that wait for their waveform pass."""

    def __init__(self, slots: int, chunk: int, admit_min: Optional[int], wave_hold: int):
        if slots < 1 or chunk < 1:
            raise ValueError("slots and chunk must be >= 1")
        admit_min = max(1, slots // 4) if admit_min is None else int(admit_min)
        if admit_min < 1:
            raise ValueError("admit_min must be >= 1")
        if wave_hold < 0:
            raise ValueError("wave_hold must be >= 0")
        self.slots, self.chunk, self.admit_min, self.wave_hold = int(slots), int(chunk), admit_min, int(wave_hold)
        self.owner: List[Optional[Tuple[Any, int]]] = [None] * self.slots      # (request, row) in each slot
        self.fifo: collections.deque = collections.deque()                     # [request, rows, next row, exclusive]
        self.missing: Dict[Any, int] = {}                                      # session request -> rows not back yet
        self.ready: List[Tuple[Any, int]] = []                                 # (request, step it became ready)
        self.stream: Dict[Any, _Stream] = {}                                   # the streaming requests not yet emitted in full
        self.fold_ready: List[Tuple[Any, int]] = []                            # folds whose rows are all back, not taken yet
        self.open = False          # a decode session is open
        self.dirty = False         # something ran since the sessions were last closed

    # -- state
    @property
    def live(self) -> int:
        return sum(o is not None for o in self.owner)

    @property
    def queued(self) -> int:
        """rows that may be admitted now: those in front of the first exclusive request"""
        n = 0
        for _, rows, nxt, exclusive in self.fifo:
            if exclusive:
                break
            n += rows - nxt
        return n

    @property
    def idle(self) -> bool:
        return not self.fifo and not self.missing and not self.ready and not self.stream

    # -- one step, in the order Scheduler.step documents
    def arrive(self, req, rows: int, exclusive: bool, step: int, folds: Optional[Sequence[int]] = None) -> None:
        """folds (a streaming request): its rows per fold, rows being in fold order; every fold has at least one row"""
        if exclusive:
            self.fifo.append([req, 0, 0, True])
        elif rows <= 0:
            self.ready.append((req, step))          # no sentence: nothing to decode
        else:
            self.fifo.append([req, int(rows), 0, False])
            self.missing[req] = int(rows)
            if folds is not None:
                if sum(folds) != rows or min(folds) < 1:
                    raise ValueError(f"folds of {list(folds)} rows for a request of {rows}")
                self.stream[req] = _Stream(folds)

    def admit(self) -> List[Tuple[Any, int, int]]:
        free = [s for s in range(self.slots) if self.owner[s] is None]
        k = admit_count(len(free), self.queued, self.slots - len(free), self.admit_min)
        out = []
        for s in free[:k]:
            e = self.fifo[0]
            self.owner[s] = (e[0], e[2])
            out.append((e[0], e[2], s))
            e[2] += 1
            if e[2] == e[1]:
                self.fifo.popleft()
        if out:
            self.open = self.dirty = True
        return out

    def finish(self, rows: Iterable[Tuple[Any, int]], step: int) -> None:
        for req, row in rows:
            self.owner[self.owner.index((req, row))] = None
            self.missing[req] -= 1
            st = self.stream.get(req)
            if st is not None:                      # a streaming request is ready fold by fold, never as a whole
                bi = st.fold[row]
                st.missing[bi] -= 1
                if st.missing[bi] == 0:
                    del st.missing[bi]
                    self.fold_ready.append((req, bi))
            if self.missing[req] == 0:
                del self.missing[req]
                if st is None:
                    self.ready.append((req, step))

    def take_folds(self) -> List[Tuple[Any, int]]:
        """the folds of streaming requests whose rows are all back, at once: a fragment does not wait for company"""
        out, self.fold_ready = self.fold_ready, []
        if out:
            self.dirty = True
        return out

    def voiced(self, req, bi: int) -> List[int]:
        """the audio of fold bi exists -> the folds to emit now, in order: bi and what waited for it, or nothing while an
        earlier fold is outstanding"""
        st = self.stream[req]
        st.voiced.add(bi)
        out = []
        while st.nxt in st.voiced:
            st.voiced.remove(st.nxt)
            out.append(st.nxt)
            st.nxt += 1
        return out

    def stream_done(self, req) -> bool:
        """every fold of the streaming request has been emitted: it is forgotten"""
        st = self.stream[req]
        if st.nxt < st.n:
            return False
        del self.stream[req]
        return True

    def wave(self, step: int, force: bool = False) -> list:
        """the requests of this step's waveform pass: all that are ready, once the oldest has waited wave_hold steps -- or at
        once when no row is live or admissible, since no company can come, or when nothing is gained by holding (`force`: the
        pass runs anyway, a streaming request's fold is in it; or, continuous_cfm, the flow-matching session is the company a
        held request would have waited for)"""
        if not self.ready:
            return []
        if not force and step - self.ready[0][1] < self.wave_hold and (self.live or self.queued):
            return []
        out = [req for req, _ in self.ready]
        self.ready = []
        self.dirty = True
        return out

    def exclusive_head(self, busy: bool = False):
        """the exclusive request to serve now, or None: it is the head of the queue and nothing is live (`busy`: the
        flow-matching session still has live or queued rows)"""
        if self.fifo and self.fifo[0][3] and not self.live and not busy:
            self.dirty = True
            return self.fifo.popleft()[0]
        return None

    def close_due(self, busy: bool = False) -> bool:
        """end of a step: nothing live, nothing queued -> the decoder is handed back (once per burst)"""
        if self.live or self.fifo or busy or not self.dirty:
            return False
        self.open = self.dirty = False
        return True

    def cancel(self, req) -> List[int]:
        """forgets the request; returns the slots its live rows held"""
        for e in list(self.fifo):
            if e[0] == req:
                self.fifo.remove(e)
        self.missing.pop(req, None)
        self.stream.pop(req, None)
        self.fold_ready = [f for f in self.fold_ready if f[0] != req]
        self.ready = [(r, t) for r, t in self.ready if r != req]
        slots = [s for s, o in enumerate(self.owner) if o is not None and o[0] == req]
        for s in slots:
            self.owner[s] = None
        return slots


class _CfmPolicy:
    """Every decision of the flow-matching session behind the decode session (`Scheduler(continuous_cfm=True)`), as host-only
    state: the FIFO of rows that wait, the row in each slot with the Euler steps it still needs, the rows each fold still
    misses and the folds each request still misses.  A row is (request, fold bi, chunk k) with its step count and whether it
    is guided; a guided row is two DiT rows."""
    TABLES = 8                 # distinct step counts among the live rows: the engine's modulation cache

    def __init__(self, rows: int, chunk: int):
        if rows < 1 or chunk < 1:
            raise ValueError("cfm_rows and cfm_chunk must be >= 1")
        self.rows, self.chunk = int(rows), int(chunk)
        self.owner: List[Optional[Tuple[Any, int, int]]] = [None] * self.rows     # (request, bi, k) in each slot
        self.left, self.steps, self.guided = [0] * self.rows, [0] * self.rows, [False] * self.rows
        self.fifo: collections.deque = collections.deque()                     # (request, bi, k, steps, guided)
        self.pending: Dict[Tuple[Any, int], int] = {}                          # (request, bi) -> rows not back yet
        self.folds: Dict[Any, int] = {}                                        # request -> folds not vocoded yet
        self.open = False

    @property
    def live(self) -> List[int]:
        return [s for s in range(self.rows) if self.owner[s] is not None]

    @property
    def dit_rows(self) -> int:
        return sum(2 if self.guided[s] else 1 for s in self.live)

    @property
    def busy(self) -> bool:
        """a row is live or queued"""
        return bool(self.fifo) or any(o is not None for o in self.owner)

    def enqueue(self, req, folds: Dict[int, Sequence[Tuple[int, bool]]], whole: bool) -> bool:
        """the rows of the encoded folds, folds[bi] = [(steps, guided), ...] (empty: the fold has no frames), join the FIFO in
        (bi, k) order; False: they bring no row at all.  whole: these are all the folds of the request, which is delivered
        when they are vocoded (`vocoded`); else one fold of a streaming request, encoded as soon as its sentences are back
        and not counted in `folds`: such a request is delivered fragment by fragment"""
        n = 0
        for bi, rows in sorted(folds.items()):
            for k, (steps, guided) in enumerate(rows):
                if int(steps) < 1:
                    raise ValueError("a row needs at least one Euler step")
                self.fifo.append((req, bi, k, int(steps), bool(guided)))
            if rows:
                self.pending[(req, bi)] = len(rows)
                n += 1
        if whole and n:
            self.folds[req] = n
        return n > 0

    def admit(self) -> List[Tuple[Any, int, int, int]]:
        """rows from the head of the FIFO into the lowest free slots while the live DiT rows fit `rows` and the distinct
        step counts fit TABLES; the head that does not fit blocks the rows behind it.  -> [(request, bi, k, slot)]"""
        out = []
        while self.fifo:
            req, bi, k, steps, guided = self.fifo[0]
            if guided and self.rows == 1 and not self.live:       # a guided row and its twin: two DiT rows at least
                self.rows = 2
                self.owner, self.left, self.steps, self.guided = [None] * 2, [0] * 2, [0] * 2, [False] * 2
            live = self.live
            if self.dit_rows + (2 if guided else 1) > self.rows or len({self.steps[s] for s in live} | {steps}) > self.TABLES:
                break
            s = min(set(range(self.rows)) - set(live))             # live rows <= live DiT rows < rows: a slot is free
            self.owner[s], self.left[s], self.steps[s], self.guided[s] = (req, bi, k), steps, steps, guided
            self.fifo.popleft()
            out.append((req, bi, k, s))
        if out:
            self.open = True
        return out

    def step(self) -> Tuple[int, List[Tuple[Tuple[Any, int, int], int]], List[Tuple[Any, int]]]:
        """one sess.step(k) of the live rows, k = min(chunk, fewest steps a live row still needs) -> (k, the rows that
        finished with their slots [((request, bi, k), slot)] in slot order, the folds whose rows are now all back)"""
        live = self.live
        k = min(self.chunk, min(self.left[s] for s in live))
        done, folds = [], []
        for s in live:
            self.left[s] -= k
            if self.left[s] == 0:
                row = self.owner[s]
                done.append((row, s))
                self.owner[s] = None
                self.pending[row[:2]] -= 1
                if self.pending[row[:2]] == 0:
                    del self.pending[row[:2]]
                    folds.append(row[:2])
        return k, done, folds

    def vocoded(self, folds: Iterable[Tuple[Any, int]]) -> list:
        """the folds went through the vocoder -> the requests whose folds are now all back, in that order"""
        out = []
        for req, _ in folds:
            if req not in self.folds:               # a streaming request: its folds are emitted one by one
                continue
            self.folds[req] -= 1
            if self.folds[req] == 0:
                del self.folds[req]
                out.append(req)
        return out

    def cancel(self, req) -> List[int]:
        """forgets the request; returns the slots its live rows held"""
        self.fifo = collections.deque(e for e in self.fifo if e[0] != req)
        self.pending = {f: n for f, n in self.pending.items() if f[0] != req}
        self.folds.pop(req, None)
        slots = [s for s in self.live if self.owner[s][0] == req]
        for s in slots:
            self.owner[s] = None
        return slots


def _run_step(pol: _Policy, cp: Optional[_CfmPolicy], be, step: int, ev: list) -> None:
    """One scheduler step behind its arrivals (`_Policy.arrive`, which the caller has done), written once for `Scheduler` and
    `plan_online`: admit, advance, finish, then the waveform pass or -- `cp` given -- the flow-matching round (encode, admit,
    Euler steps, vocode), fragments and deliveries, then the exclusive requests that are due, then the close of an idle
    burst.  The decisions are the policies', the events are appended to `ev` here and nowhere else, and everything else is a
    method of the backend `be` (`_Replay` lists them).  A stage that raises fails the requests it was working on
    (`be._fail(requests, exception)`, which takes their rows out of both policies with `cancel`) and nobody else; a backend
    may also fail requests inside a stage, so no request is expected to be still known after one."""
    def attempt(reqs, stage, *args):
        try:
            return stage(*args)
        except Exception as e:                                          # noqa: BLE001 -- the result of the stage's requests
            be._fail(reqs, e)                                           # and the stage's result is None

    def fragments(voiced):
        """the audio of these folds exists: the fragments that are due, per request in fold order"""
        due = [(r, b) for r, bi in voiced if r in pol.stream for b in pol.voiced(r, bi)]
        if due:
            ends = [r for r in dict.fromkeys(r for r, _ in due) if pol.stream_done(r)]
            for r, b in attempt(sorted({r for r, _ in due}), be._emit, due, ends) or ():
                ev.append(("fragment", r, b))

    def encode(r, bi=None):
        """request r (or its fold bi) joins the flow-matching FIFO -> True: it brings no row and has nothing to wait for"""
        return attempt([r], lambda: not cp.enqueue(r, be._encode(r, bi), whole=bi is None))

    admitted = pol.admit()
    if admitted:
        be._admit(admitted)
        ev.append(("admit", admitted))
    if pol.live:
        done = be._advance(pol.chunk)
        ev.append(("advance", pol.chunk, done))
        pol.finish(done, step)
    if cp is None:
        sfolds = pol.take_folds()
        ready = pol.wave(step, force=bool(sfolds))
        if ready or sfolds:
            ev.append(("wave", ready) + ((sfolds,) if sfolds else ()))
            attempt(ready + sorted({r for r, _ in sfolds}), be._wave, ready, sfolds)
            be._deliver(ready)
            fragments(sfolds)
    else:
        deliver = [r for r in pol.wave(step, force=True) if encode(r)]
        voiced = [(r, bi) for r, bi in pol.take_folds() if r in pol.stream and encode(r, bi)]
        admitted = cp.admit()
        if admitted:
            ev.append(("cfm_admit", admitted))
            attempt(sorted({r for r, _, _, _ in admitted}), be._cfm_admit, admitted)
        if cp.live:
            holders = sorted({cp.owner[s][0] for s in cp.live})
            k, done, folds = cp.step()
            ev.append(("cfm_step", k, [row for row, _ in done]))
            mels = attempt(holders, be._cfm_step, k, done)
            if mels is None:
                cp.open = False                     # the session went with the step; queued rows open the next one
            elif folds:
                ev.append(("vocode", folds))
                attempt(sorted({r for r, _ in folds}), be._vocode, folds, mels)
                deliver += cp.vocoded(folds)
                voiced += [f for f in folds if f[0] in pol.stream]
        fragments(voiced)
        deliver = be._deliver(deliver)
        if deliver:
            ev.append(("deliver", deliver))

    def close():
        pol.open = False
        if cp is not None:
            cp.open = False
        be._close_sessions()
        ev.append(("close",))
    busy = cp is not None and cp.busy
    while True:
        was_open = pol.open or (cp is not None and cp.open)
        r = pol.exclusive_head(busy)
        if r is None:
            break
        if was_open:
            close()
        ev.append(("exclusive", r))
        be._exclusive(r)
    if pol.close_due(busy):
        close()


class _Replay:
    """`plan_online`'s backend: the stages of `_run_step` with nothing behind them but the rows' `lengths`, counted down, and
    the flow-matching rows of `cfm_folds`, looked up.  Its docstrings are the contract of each backend method."""

    def __init__(self, slots: int, lengths: Sequence[int], first: Dict[int, int], cfm_folds):
        self.lengths, self.first, self.cfm_folds = lengths, first, cfm_folds
        self.row: List[Optional[Tuple[int, int]]] = [None] * slots
        self.left = [0] * slots

    def _admit(self, admitted) -> None:
        """[(request, row, slot)] take their slots in the decode session"""
        for r, row, s in admitted:
            self.row[s], self.left[s] = (r, row), int(self.lengths[self.first[r] + row])

    def _advance(self, chunk: int) -> List[Tuple[int, int]]:
        """the live rows go `chunk` steps -> the (request, row) that finished, in slot order"""
        done = []
        for s, row in enumerate(self.row):
            if row is not None:
                self.left[s] -= min(chunk, self.left[s])
                if self.left[s] == 0:
                    done.append(row)
                    self.row[s] = None
        return done

    def _encode(self, r, bi):
        """-> {bi: [(steps, guided), ...]}: the flow-matching rows of request r's folds, or of its fold bi alone"""
        return dict(enumerate(self.cfm_folds[r])) if bi is None else {bi: self.cfm_folds[r][bi]}

    def _cfm_step(self, k: int, done):
        """k Euler steps; `done` [((request, bi, k), slot)] finished with them -> their mels for `_vocode`, never None"""
        return ()

    def _emit(self, due, ends):
        """the fragments `due` [(request, bi)]; the requests `ends` have their last one among them -> the fragments emitted"""
        return due

    def _deliver(self, reqs):
        """the requests are finished and answered -> those that were still outstanding"""
        return reqs

    def _launch(self, *args) -> None:
        """the stages that return nothing: `_wave(ready, sfolds)`, the waveform pass of the requests `ready` and the folds
        `sfolds` [(request, bi)] of streaming requests; `_cfm_admit([(request, bi, k, slot), ...])` into the flow-matching session;
        `_vocode(folds, mels)`, the completed folds [(request, bi)]; `_exclusive(request)`, alone; `_close_sessions()`, both"""
    _wave = _cfm_admit = _vocode = _exclusive = _close_sessions = _launch

    def _fail(self, reqs, exc: BaseException) -> None:
        """a stage working on these requests raised: they get `exc` as their result and leave both policies (`cancel`).
        Nothing fails in a replay but its arguments (a row of no Euler steps), and that is the caller's exception"""
        raise exc


def plan_online(arrivals: Sequence[int], rows_per_request: Sequence[int], lengths: Sequence[int], slots: int, chunk: int,
                admit_min: Optional[int] = None, wave_hold: int = 0, exclusive=(), with_steps: bool = False,
                cfm_folds: Optional[Sequence[Sequence[Sequence[Tuple[int, bool]]]]] = None, cfm_rows: Optional[int] = None,
                cfm_chunk: Optional[int] = None, streaming: Optional[Dict[int, Sequence[int]]] = None):
    """The schedule `Scheduler` follows, as a pure function.  Request r is submitted in front of step arrivals[r] (requests
    arriving in the same step keep their order) and brings rows_per_request[r] rows; `lengths` lists, request after request and
    row after row, how many further steps each row needs after its step 0 (0: it ends at its admission), as `plan_continuous`
    takes them.  The requests named in `exclusive` bring no rows (their entry of rows_per_request is not read).  Returns the
    events ("admit", [(req, row, slot), ...]), ("advance", chunk, [(req, row) reported finished, in slot order]),
    ("wave", [reqs]), ("exclusive", req) and ("close",); with_steps=True, (step, event) pairs.  With every arrival at step 0 and
    no exclusive request the admit / advance events are `plan_continuous`'s.
    `cfm_folds` given (with `cfm_rows` and `cfm_chunk`): the schedule of `Scheduler(continuous_cfm=True)`.  cfm_folds[r][bi] lists
    the flow-matching rows of request r's fold bi as (sample_steps, guided) pairs -- an empty list is a fold without frames, an
    exclusive request's entry is not read.  No ("wave", ...) is emitted; instead, after the advance of a step: ("cfm_admit",
    [(req, bi, k, slot), ...]), ("cfm_step", k, [(req, bi, k) finished, in slot order]), ("vocode", [(req, bi) of the folds
    completed in this step]) and ("deliver", [reqs]): the requests without rows that became ready in this step, then those
    whose last fold was vocoded in it.  An exclusive request waits until neither session has a live or queued row, and
    ("close",) closes both sessions.  Without `cfm_folds` the trace is the one described above.
    `streaming`: {r: the rows of each of its folds} names the streaming requests (a request also named in `exclusive` stays
    exclusive and its entry is not read).  Such a request is never in a ("wave", ...) or ("deliver", ...) list: a fold whose
    rows are all back goes into that step's pass -- ("wave", [reqs], [(req, bi), ...]), the pass fires at once and every ready
    request rides along -- or, with `cfm_folds`, its rows join the flow-matching FIFO at once, so the ("cfm_admit", ...) events
    are fold-granular.  ("fragment", req, bi) follows the pass (the ("vocode", ...) event) that made fold bi's audio, once every
    earlier fold of the request has been emitted: bi = 0, 1, ... per request.  With no streaming request the trace is
    unchanged."""
    n = len(arrivals)
    if cfm_folds is not None and (cfm_rows is None or cfm_chunk is None or len(cfm_folds) != n):
        raise ValueError("cfm_folds needs cfm_rows, cfm_chunk and one entry per request")
    cp = _CfmPolicy(cfm_rows, cfm_chunk) if cfm_folds is not None else None
    if len(rows_per_request) != n:
        raise ValueError(f"{len(rows_per_request)} row counts for {n} arrivals")
    excl = set(exclusive)
    first, total = {}, 0
    for r in range(n):
        first[r] = total
        total += 0 if r in excl else int(rows_per_request[r])
    if total != len(lengths):
        raise ValueError(f"{len(lengths)} lengths for {total} rows")
    streaming = {int(r): [int(k) for k in f] for r, f in (streaming or {}).items() if r not in excl}
    for r, f in streaming.items():
        if sum(f) != int(rows_per_request[r]):
            raise ValueError(f"request {r}: folds of {f} rows, {rows_per_request[r]} rows")
    pol = _Policy(slots, chunk, admit_min, wave_hold)
    order = sorted(range(n), key=lambda r: (int(arrivals[r]), r))
    be = _Replay(pol.slots, lengths, first, cfm_folds)
    trace, nxt, step = [], 0, 0
    while nxt < n or not pol.idle or (cp is not None and cp.busy):
        if pol.idle and not (cp is not None and cp.busy) and int(arrivals[order[nxt]]) > step:
            step = int(arrivals[order[nxt]])            # nothing to do until the next arrival
        while nxt < n and int(arrivals[order[nxt]]) <= step:
            r = order[nxt]
            pol.arrive(r, 0 if r in excl else int(rows_per_request[r]), r in excl, step, streaming.get(r) or None)
            nxt += 1
        ev: list = []
        _run_step(pol, cp, be, step, ev)
        trace += [(step, e) for e in ev] if with_steps else ev
        step += 1
    return trace


class Scheduler:
    """The step-driven scheduler over a loaded `TTS` pipeline.  Not thread-safe: one thread calls it (`Server`'s loop).
    slots: rows of the decode session (default: the decoder's max_batch); chunk: steps per advance; admit_min: as `admit_count`
    (default max(1, slots // 4)); wave_hold: steps a finished request may wait for others to share its waveform pass.
    shared_hubert / shared_bert / shared_sv / device_frontend / shared_vocoder: as `run_batch`'s keywords, applied to the
    requests one step takes in (front-ends) and to the requests one step finishes (vocoder).
    continuous_cfm (v3 / v4 only, off by default): the waveform stage is a second open session behind the first.  A request
    whose sentences are all back is encoded at once (`TTS._cfm_encode`) and its flow-matching rows join a FIFO; every step admits
    rows from its head into the free slots of ONE flow-matching session (`CFMSession`, per-row step count, guidance rate and
    LoRA slot), runs min(cfm_chunk, fewest steps a live row still needs) Euler steps, fetches the rows that finished with one
    `fetch_mel` call, vocodes the folds whose rows are all back and delivers the requests whose folds are all back.  cfm_rows:
    the session's DiT rows (default min(tts.cfm_max_rows, 64); a guided row counts 2, and 1 is raised to 2 when a guided row
    waits); cfm_chunk: the most Euler steps one scheduler step runs before it takes in new arrivals.  wave_hold does not apply
    to this path: the session is the company a held request would have waited for.  Without the keyword the scheduler issues
    exactly the launches it issued before the keyword existed.
    mixed_limits (off by default): prompt-free requests, parallel_infer=False requests, "best_of" requests and requests with a
    row short of arena room are no longer exclusive.  Their rows enter the decode session with limits of their own
    (plan_batch(mixed_limits=True): EOS horizon 11 for the naive and prompt-free ones, the arena-bound budget for the short
    ones), a prompt-free row without a prompt, a "best_of" sentence as its n candidate rows; the session is opened with per-row
    limits and log-probabilities, and a sentence is back when all its candidates are (choose_candidate then fills its tokens
    and the request's `candidates`, as TTS._ar_stage does).  Only a request with a row that has no room at all (budget < 1)
    stays exclusive: run_batch([request]) raises its own error for it alone.  Without the keyword nothing changes."""

    def __init__(self, tts, slots: Optional[int] = None, chunk: int = 32, admit_min: Optional[int] = None, wave_hold: int = 0,
                 shared_hubert: bool = True, shared_bert: bool = True, shared_sv: bool = False, device_frontend: bool = False,
                 shared_vocoder: bool = False, continuous_cfm: bool = False, cfm_rows: Optional[int] = None, cfm_chunk: int = 2,
                 mixed_limits: bool = False):
        if tts.t2s_model is None or tts.vits_model is None:
            raise RuntimeError("init_t2s_weights / init_vits_weights first")
        if continuous_cfm and not getattr(tts.configs, "use_vocoder", False):
            raise ValueError("continuous_cfm=True is the flow-matching stage of v3 / v4: this model has no vocoder")
        if device_frontend and not (shared_hubert or shared_sv):
            raise ValueError("device_frontend=True is the front-end of the shared make_voices call: pass shared_hubert=True or shared_sv=True too")
        self.tts = tts
        slots = tts.t2s_model.max_batch if slots is None else int(slots)
        if slots > tts.t2s_model.max_batch:
            raise ValueError(f"{slots} slots, the decoder's max_batch is {tts.t2s_model.max_batch}")
        self._pol = _Policy(slots, chunk, admit_min, wave_hold)
        self._front = dict(shared_hubert=bool(shared_hubert), shared_bert=bool(shared_bert), shared_sv=bool(shared_sv),
                           device_frontend=bool(device_frontend))
        self._shared_vocoder = bool(shared_vocoder)
        self._mixed_limits = bool(mixed_limits)
        self._cands: Dict[Tuple[int, int, int], Dict[int, tuple]] = {}  # (ticket, bi, j) -> candidate -> (its dict, y), until all are back
        self._cpol: Optional[_CfmPolicy] = None
        if continuous_cfm:
            from ._lib import CFM_SESSION_MAX_ROWS
            self._cpol = _CfmPolicy(min(int(tts.cfm_max_rows), CFM_SESSION_MAX_ROWS) if cfm_rows is None else int(cfm_rows), cfm_chunk)
            if self._cpol.rows > CFM_SESSION_MAX_ROWS:
                raise ValueError(f"cfm_rows {self._cpol.rows}: a flow-matching session holds at most {CFM_SESSION_MAX_ROWS} DiT rows")
        self._cfm = None                            # the open CFMSession
        self._cfm_req: Dict[int, dict] = {}         # ticket -> dict(vk, fold_in {bi: (rows, lens, pad_len)}, mel {bi: packed mel})
        self._cfm_prompts: Dict[tuple, tuple] = {}  # _prompt_features() of the voices of the requests in _cfm_req
        self._inbox: List[Tuple[int, dict]] = []
        self._requests: Dict[int, dict] = {}        # ticket -> request (exclusive) or plan (session), until delivered
        self._rows: Dict[int, List[dict]] = {}      # ticket -> its rows in queue order: dict(bi, j, key, sampling)
        self._where: Dict[int, Tuple[int, int]] = {}    # session ticket -> (ticket, row)
        self._done: List[Tuple[int, Any]] = []      # results the running step, or the next one, returns (cancel adds between steps)
        self._frags: List[Tuple[int, int, Any]] = []    # (ticket, bi, (sr, audio)) emitted in the last step (take_fragments)
        self._ses = None
        self._next, self._step = 0, 0
        self._closed = False
        self.sessions: list = []                    # every closed T2SSession, in order (history, modes, adopt times)
        self.stats: Dict[str, Any] = dict(steps=0, admissions=0, rows=0, advances=0, waves=0, exclusive=0, sessions=0, released=0,
                                          occupancy=[], events=[], tickets={})
        if continuous_cfm:                          # admissions, rows, Euler steps, live DiT rows per step call, vocoder calls, and
            self.stats.update(cfm_admissions=0, cfm_rows=0, cfm_steps=0, cfm_occupancy=[], vocoder_calls=0, cfm_sessions=0,
                              cfm_released=0, cfm_folds={})     # per ticket the rows per fold as plan_online takes them

    # -- public
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    @property
    def idle(self) -> bool:
        return not self._inbox and not self._done and self._pol.idle and not (self._cpol is not None and self._cpol.busy)

    def submit(self, request: dict) -> int:
        """enqueues the request (the dict `run_batch` takes) for the next step; returns its ticket.  No GPU work."""
        if self._closed:
            raise RuntimeError("the scheduler is closed")
        t = self._next
        self._next += 1
        self._inbox.append((t, request))
        self.stats["tickets"][t] = [self._step, None, None]
        return t

    def cancel(self, ticket: int) -> bool:
        """drops the request's queued rows and releases its live ones -- in the decode session and, continuous_cfm, in the
        flow-matching session, with its partial fold buffers and its voice's cached prompt features; its result, returned by
        the next step, is CancelledError.  False if the ticket is not outstanding (unknown, or delivered)."""
        if any(t == ticket for t, _ in self._inbox):
            self._inbox = [(t, r) for t, r in self._inbox if t != ticket]
        elif ticket in self._requests:
            self._forget(ticket)
        else:
            return False
        self._done.append((ticket, CancelledError()))
        return True

    def _forget(self, ticket: int) -> None:
        """drops an outstanding request: queued rows, live rows of both sessions (released), fold buffers, its plan"""
        slots = self._pol.cancel(ticket)
        if slots:
            self._ses.release_slots(slots)
            self._count(released=len(slots))
            self.stats["events"].append(("release", slots))
        self._where = {k: v for k, v in self._where.items() if v[0] != ticket}
        self._drop_cfm(ticket)
        self._requests.pop(ticket)
        self._rows.pop(ticket, None)
        self._cands = {k: v for k, v in self._cands.items() if k[0] != ticket}

    def take_fragments(self) -> List[Tuple[int, int, Any]]:
        """the fragments the last step emitted, in emission order: [(ticket, bi, (sr, int16 audio))] -- per streaming request
        bi = 0, 1, ...; the request's final result (the list of all of them) comes from the step that emits the last one"""
        out, self._frags = self._frags, []
        return out

    def close(self) -> None:
        """drops what is outstanding (no step will return it) and closes the sessions: `tts.run` / `run_batch` work again"""
        for t in [t for t, _ in self._inbox] + list(self._requests):
            self.cancel(t)
        self._done = []
        self._close_sessions()
        self._closed = True

    def step(self) -> List[Tuple[int, Any]]:
        """One round: intake, admit, advance, finish (continuous_cfm: encode, flow-matching admit, step, fetch, vocode,
        deliver), exclusive requests, close when idle (`_run_step`, behind the intake).  Returns the
        (ticket, result) pairs of the requests that ended in it; a result is (sr, int16 audio), the list of fragments of a
        `return_fragment` request (returned by the step that emits the last one; `take_fragments` has each as it is made), or
        the exception the request raised."""
        import torch
        self._frags = []
        with torch.no_grad():
            self._intake(self._done)
            _run_step(self._pol, self._cpol, self, self._step, self.stats["events"])
        out, self._done = self._done, []
        for t, _ in out:
            self.stats["tickets"][t][2] = self._step
        self._step += 1
        self.stats["steps"] = self._step
        return out

    def _count(self, **counts: int) -> None:
        for name, n in counts.items():
            self.stats[name] += n

    # -- the step: what `_run_step` calls (`_Replay` says what each does for the schedule), behind the intake
    def _resolve(self, taken: List[Tuple[int, dict]], out: list) -> List[Tuple[int, dict]]:
        """voices and texts of one intake through the shared front-ends, as ONE call each; a call that raises is repeated
        request by request, so that only the request at fault gets the exception"""
        tts, f = self.tts, self._front
        calls = []
        if f["shared_bert"]:
            calls.append(tts._with_shared_segments)
        if f["shared_hubert"] or f["shared_sv"]:
            calls.append(lambda reqs: tts._with_shared_voices(reqs, shared_sv=f["shared_sv"], device_frontend=f["device_frontend"]))
        for call in calls:
            if not taken:
                break
            try:
                taken = list(zip([t for t, _ in taken], call([r for _, r in taken])))
            except Exception:                                           # noqa: BLE001 -- found again below, per request
                kept = []
                for t, r in taken:
                    try:
                        kept.append((t, call([r])[0]))
                    except Exception as e:                              # noqa: BLE001 -- the request's own result
                        out.append((t, e))
                taken = kept
        return taken

    def _intake(self, out: list) -> None:
        taken, self._inbox = self._inbox, []
        # a streaming request is planned like any other (the planner's `fragments` keyword is passed for it alone)
        taken = [(t, dict(r, return_fragment=True) if r.get("return_fragment") or r.get("streaming_mode") else r) for t, r in taken]
        plans = {}
        for t, req in self._resolve(taken, out):
            try:
                plans[t] = (req, self.tts._plan_request(req, **({"fragments": True} if req.get("return_fragment") else {}),
                                                        **({} if req.get("timestamps") in (None, False) else {"timestamps": True})))
            except Exception as e:                                      # noqa: BLE001 -- the request's own result
                out.append((t, e))
        for t, (req, pl) in sorted(plans.items()):                      # arrival order
            rows = self._session_rows(pl)
            if rows is None:
                self._requests[t] = req
                self._pol.arrive(t, 0, True, self._step)
            else:
                pl["preds"] = [[None] * len(item["all_phones"]) for item in pl["data"]]
                pl["idxs"] = [[None] * len(item["all_phones"]) for item in pl["data"]]
                pl["kept"] = [None] * len(pl["data"])                   # per fold, filled when its sentences are back (_keep)
                self._requests[t], self._rows[t] = pl, rows
                folds = None
                if pl["opts"]["return_fragment"]:                       # delivered fold by fold: (bi, j) order is fold order
                    pl["stream"] = []
                    folds = [sum(e["bi"] == bi for e in rows) for bi in range(len(pl["data"]))]     # candidate rows included
                self._pol.arrive(t, len(rows), False, self._step, folds or None)

    def _budget(self) -> int:
        from .TTS_infer_pack.TTS import early_stop_num
        return min(1500, int(early_stop_num(self.tts.configs)) + 1)

    def _session_rows(self, pl: dict) -> Optional[List[dict]]:
        """the request's rows in (bi, j) order with plan_batch's keys and sampling tuples -- or None: the request is exclusive
        (prompt-free, the naive loop, "best_of" candidates, or a row that does not fit the K/V arena with the full step budget).
        mixed_limits: all of those bring rows too, with "limits", "no_prompt" and, for candidates, "cand" as plan_batch gives
        them, in (bi, j, candidate) order; None only if a row has no room at all."""
        if self._mixed_limits:
            rows = [e for launch in self.tts.plan_batch([pl], mixed_sampling=True, mixed_limits=True) for e in launch]
            if any(e["limits"][2] < 1 for e in rows):
                return None
            return sorted(rows, key=lambda e: (e["bi"], e["j"], e.get("cand", 0)))
        if pl["no_prompt"] or not pl["opts"]["parallel_infer"] or "best_of" in pl["opts"]:
            return None
        rows = [e for launch in self.tts.plan_batch([pl], mixed_sampling=True) for e in launch]
        if any(e["len"] + 2 + self._budget() > self.tts.t2s_model.max_seq for e in rows):
            return None
        return sorted(rows, key=lambda e: (e["bi"], e["j"]))

    def _admit(self, admitted: List[Tuple[int, int, int]]) -> None:
        from .TTS_infer_pack.TTS import early_stop_num
        rows = []
        for t, row, _ in admitted:
            pl, e = self._requests[t], self._rows[t][row]
            item = pl["data"][e["bi"]]
            rows.append(dict(x=item["all_phones"][e["j"]], bert=item["all_bert_features"][e["j"]],
                             prompt=None if e.get("no_prompt") else pl["voice"]["prompt_semantic"].view(-1), key=e["key"],
                             sampling=e["sampling"]))
            if self._mixed_limits:
                rows[-1]["limits"] = e["limits"]
            if self.stats["tickets"][t][1] is None:
                self.stats["tickets"][t][1] = self._step
        if self._ses is None:
            k, p, temp, rp = rows[0]["sampling"]        # placeholders: every row brings its own tuple
            self._ses = self.tts.t2s_model.open_session(self._pol.slots, k, p, temp, rp, early_stop_num(self.tts.configs), 1,
                                                        self._budget(), row_sampling=True,
                                                        **(dict(row_limits=True, logprobs=True) if self._mixed_limits else {}))
            self._count(sessions=1)
        tickets = self._ses.admit(rows, slots=[s for _, _, s in admitted])
        for st, (t, row, _) in zip(tickets, admitted):
            self._where[st] = (t, row)
        self._count(admissions=1, rows=len(rows))

    def _advance(self, chunk: int) -> List[Tuple[int, int]]:
        self.stats["occupancy"].append(self._pol.live)
        done = []
        for st, y, n in self._ses.advance(chunk):
            t, row = self._where.pop(st)
            e = self._rows[t][row]
            pl = self._requests[t]
            done.append((t, row))
            if "cand" in e:                                             # a sentence is back when all its candidates are
                from .TTS_infer_pack.TTS import choose_candidate
                c = dict(tokens=y[-n:] if n > 0 else y[:0], logprobs=self._ses.logprobs[st].cpu().numpy(), n=n, cut=self._ses.cut[st])
                by_c = self._cands.setdefault((t, e["bi"], e["j"]), {})
                by_c[e["cand"]] = (c, y)
                if len(by_c) < pl["opts"]["best_of"]:
                    continue
                del self._cands[(t, e["bi"], e["j"])]
                k, rec = choose_candidate(pl["opts"], [by_c[c_][0] for c_ in sorted(by_c)])
                y, n = by_c[k][1], by_c[k][0]["n"]
                pl.setdefault("candidates", [[None] * len(item["all_phones"]) for item in pl["data"]])[e["bi"]][e["j"]] = rec
            pl["preds"][e["bi"]][e["j"]], pl["idxs"][e["bi"]][e["j"]] = y, (0 if e.get("no_prompt") else n)
        self._count(advances=1)
        return done

    def _keep(self, pl: dict, folds: Iterable[int]) -> None:
        """the sentences of these folds are back: their AR output without the prompts, as the waveform stages take it"""
        for bi in folds:
            pl["kept"][bi] = self.tts._kept_tokens(pl["preds"][bi], pl["idxs"][bi], pl["no_prompt"])

    def _wave(self, ready: List[int], sfolds: Sequence[Tuple[int, int]]) -> None:
        """the ready requests through run_batch's waveform stages, called with the ready subset (a stage that raises fails
        the requests of this pass).  sfolds: the ready folds of streaming requests, which go through the same pass -- the
        stage is then restricted to them and to every fold of the ready requests."""
        tts = self.tts
        self._count(waves=1)
        plans = [self._requests[t] for t in ready]
        streams = sorted({t for t, _ in sfolds})
        for pl in plans:
            self._keep(pl, range(len(pl["data"])))
        kw = {}
        if sfolds:
            at = {t: len(plans) + n for n, t in enumerate(streams)}
            for t, bi in sfolds:
                self._keep(self._requests[t], [bi])
            kw["folds"] = [(r, bi) for r, pl in enumerate(plans) for bi in range(len(pl["data"]))] + [(at[t], bi) for t, bi in sfolds]
        tts._wait_stream()
        tts._output_sr()                                                # a model without its vocoder fails the whole pass
        if tts.configs.use_vocoder:
            tts._shared_cfm_stage(plans + [self._requests[t] for t in streams], shared_vocoder=self._shared_vocoder, **kw)
        else:
            tts._shared_sovits_stage(plans + [self._requests[t] for t in streams], **kw)

    def _deliver(self, reqs: Iterable[int]) -> List[int]:
        """the requests that are still outstanding, each through _finish_request; a streaming request that reaches it has no
        sentence at all, and run() yields that second of silence as its one fragment"""
        tts = self.tts
        reqs = [t for t in reqs if t in self._requests]                 # a failed stage has answered for the others
        for t in reqs:
            pl = self._requests.pop(t)
            self._rows.pop(t, None)
            self._drop_cfm(t)
            try:
                result = tts._finish_request(pl, tts._output_sr())
                if pl["opts"]["return_fragment"]:
                    self._frags.append((t, 0, result))
                    result = [result]
                self._done.append((t, result))
            except Exception as e:                                      # noqa: BLE001 -- the request's own result
                self._done.append((t, e))
        return reqs

    def _emit(self, due: Sequence[Tuple[int, int]], ends: Iterable[int]) -> List[Tuple[int, int]]:
        """the fragments that are due -- folds of streaming requests whose audio exists (a fold no shared stage took goes
        through _synthesize_batch here, as in _finish_request), per request in fold order -- are what run() yields for them,
        audio_postprocess([frags], ...), all through ONE postprocess_fragments call (super_sampling fragments:
        audio_postprocess each, AP-BWE runs per fragment).  Fragments whose requests name an output format ("sample_rate",
        "encoding") are grouped by it: one postprocess_fragments call, that is one gsv_postprocess_groups_rate launch pair, per
        format, the default format as before.  A request of `ends`, whose last fragment is among them, gets the
        list of all of them as its result.  -> the fragments emitted"""
        tts = self.tts
        got: Dict[Tuple[int, int], Any] = {}
        batch: List[Tuple[int, int]] = []
        for t, b in due:
            if t not in self._requests:
                continue
            pl = self._requests[t]
            o = pl["opts"]
            try:
                if pl["frags"][b] is None or any(f is None for f in pl["frags"][b]):
                    with tts._with_prompt_cache(dict(pl["voice"])) as voice:
                        tts._synthesize_fold(pl, b, tts._voice_refer(voice))
                if o["super_sampling"]:
                    tts._wait_stream()
                    got[(t, b)] = tts.audio_postprocess([pl["frags"][b]], tts._output_sr(), None, o["speed_factor"], False,
                                                        o["fragment_interval"], True, **tts._format_kw(o))
                else:
                    batch.append((t, b))
            except Exception as e:                                      # noqa: BLE001 -- the request's own result
                self._fail([t], e)
        classes: Dict[Tuple[Optional[int], Optional[str]], List[Tuple[int, int]]] = {}
        for t, b in batch:
            if t in self._requests:
                o = self._requests[t]["opts"]
                classes.setdefault((o.get("sample_rate"), o.get("encoding")), []).append((t, b))
        for (rate, enc), batch in classes.items():
            batch = [(t, b) for t, b in batch if t in self._requests]   # a class before this one may have failed its requests
            try:
                if batch:
                    tts._wait_stream()
                    sr = tts._output_sr()
                    kw = {k: v for k, v in (("sample_rate", rate), ("encoding", enc)) if v is not None}
                    # "loudness" is per fragment inside the one call of its format
                    loud = [None if "loudness" not in o else (o["loudness"], o["loudness_scope"], o["loudness_peak"])
                            for o in (self._requests[t]["opts"] for t, _ in batch)]
                    if any(c is not None for c in loud):
                        kw["loudness"] = loud
                    audios = tts.postprocess_fragments([(self._requests[t]["frags"][b], self._requests[t]["opts"]["fragment_interval"])
                                                        for t, b in batch], **kw)
                    got.update({f: (sr if rate is None else rate, a) for f, a in zip(batch, audios)})
            except Exception as e:                                      # noqa: BLE001 -- the requests of this launch
                self._fail(sorted({t for t, _ in batch}), e)
        emitted = [f for f in due if f[0] in self._requests]
        for t, b in emitted:
            pl = self._requests[t]
            if "timestamps" in pl["opts"]:      # speech marks of the fragment, as run() yields them: times
                from .timestamps import build_marks       # relative to the fragment, "offset" = its start in the request's stream
                sents, sr = tts._fold_sentences(pl, b), tts._output_sr()
                gap = int(tts.configs.sampling_rate * pl["opts"]["fragment_interval"])
                off = pl.get("ts_offset", 0)
                got[(t, b)] = tuple(got[(t, b)]) + ([dict(m, offset=off / sr) for m in build_marks(sents, sr, gap)],)
                pl["ts_offset"] = off + sum(s["n_samples"] + gap for s in sents)
            pl["stream"].append(got[(t, b)])
            pl["frags"][b] = []                                         # the waveforms are delivered: the device memory goes
            self._frags.append((t, b, got[(t, b)]))
        for t in ends:                                                  # after the last fragment: the request's result
            if t in self._requests:
                pl = self._requests.pop(t)
                self._rows.pop(t, None)
                self._drop_cfm(t)
                self._done.append((t, pl["stream"]))
        return emitted

    def _exclusive(self, t: int) -> None:
        self._count(exclusive=1)
        req = self._requests.pop(t)
        try:
            if req.get("return_fragment") or req.get("streaming_mode"):
                frags = list(self.tts.run(dict(req, return_fragment=True)))
                self._done.append((t, frags))
                self._frags += [(t, bi, f) for bi, f in enumerate(frags)]
            else:
                self._done.append((t, self.tts.run_batch([req])[0]))
        except Exception as e:                                          # noqa: BLE001 -- the request's own result
            self._done.append((t, e))

    # -- continuous_cfm: the second session (class docstring)
    def _encode(self, t: int, fold: Optional[int]) -> Dict[int, List[Tuple[int, bool]]]:
        """the first half of the shared flow-matching stage for one request -- or for that one fold of a streaming request,
        whose sentences are back -> the rows of each fold it encoded, which join the FIFO"""
        tts, pl = self.tts, self._requests[t]
        folds = range(len(pl["data"])) if fold is None else [fold]
        self._keep(pl, folds)
        tts._wait_stream()
        _, fold_in, voice_of = tts._cfm_encode([pl], self._cfm_prompts, **({} if fold is None else {"folds": [(0, fold)]}))
        rows: Dict[int, List[Tuple[int, bool]]] = {bi: [] for bi in folds}
        for (_, bi, _), steps, rate in tts.plan_cfm_rows([pl]):         # only the folds just encoded have frames
            rows[bi].append((steps, rate > 0.0))
        c = self._cfm_req.setdefault(t, dict(vk=voice_of[0], fold_in={}, mel={}))
        c["fold_in"].update({bi: v for (_, bi), v in fold_in.items()})
        self.stats["cfm_folds"].setdefault(t, [[] for _ in pl["data"]])
        for bi in folds:
            self.stats["cfm_folds"][t][bi] = rows[bi]
        return rows

    def _cfm_admit(self, admitted: List[Tuple[int, int, int, int]]) -> None:
        from .module.models import CFM
        tts, cp = self.tts, self._cpol
        import torch
        rows = [(self._requests[t], self._cfm_req[t], bi, k) for t, bi, k, _ in admitted]
        mu = torch.cat([c["fold_in"][bi][0][k:k + 1] for _, c, bi, k in rows], 0)
        if self._cfm is not None and self._cfm.rows_cap != cp.rows:      # 1 raised to 2 for a guided row: nothing is live
            self._close_cfm()
        if self._cfm is None:
            self._cfm = tts.vits_model.cfm.open_session(cp.rows, int(mu.shape[1]))
            self._count(cfm_sessions=1)
        names = [pl["opts"].get("lora_voice") for pl, _, _, _ in rows]
        rates = [float(pl["opts"].get("inference_cfg_rate", 0)) for pl, _, _, _ in rows]
        guided = [cp.guided[s] for _, _, _, s in admitted]
        self._cfm.admit(mu, [self._cfm_prompts[c["vk"]][3] for _, c, _, _ in rows], [int(pl["opts"]["sample_steps"]) for pl, _, _, _ in rows],
                        [r if g else 0.0 for r, g in zip(rates, guided)],
                        seeds=[CFM.row_seed(pl["actual_seed"] + bi, k) for pl, _, bi, k in rows],
                        adapters=[None if n is None else tts._lora_voice(n)[1] for n in names] if any(names) else None,
                        slots=[s for _, _, _, s in admitted])
        self._count(cfm_admissions=1, cfm_rows=len(admitted))

    def _cfm_step(self, k: int, done: list) -> Dict[Tuple[int, int], Any]:
        """k Euler steps of the live rows and ONE fetch of those that finished (`done`, with their slots) -> the packed mel of
        every fold that is now complete.  A step that raises takes the session with it: every request with a live row fails."""
        cp = self._cpol
        self.stats["cfm_occupancy"].append(cp.dit_rows + sum(2 if cp.guided[s] else 1 for _, s in done))   # live at its start
        try:
            finished = self._cfm.step(k)
            assert finished == sorted(s for _, s in done), f"the session reports slots {finished}, the policy {done}"
            self._count(cfm_steps=k)
            return self._fetch(done) if done else {}
        except Exception:
            self._close_cfm()
            raise

    def _fetch(self, done: list) -> Dict[Tuple[int, int], Any]:
        """ONE fetch_mel call for the slots that finished in this step, into a matrix of this step [mel][sum of the rows' frames]
        in (request, bi, k) order -- so the rows of a fold that finished together are its packed mel [mel][chunks * chunk_len],
        _fold_mel's layout, as they stand.  A fold whose rows come back in several steps is put together in a buffer of its own.
        -> {(request, bi): the packed mel [1, mel, chunks * chunk_len] of every fold that is complete}"""
        import torch
        from .TTS_infer_pack.TTS import spec_max, spec_min
        sess = self._cfm
        order = sorted(done)                                            # ((t, bi, k), slot)
        lens = [sess.T - int(self._cfm_prompts[self._cfm_req[t]["vk"]][3].shape[2]) for (t, _, _), _ in order]
        col0 = [sum(lens[:i]) for i in range(len(order))]
        stage = torch.empty(sess.cfm.in_channels, sum(lens), dtype=torch.float32, device=sess.cfm.estimator.device)
        sess.fetch_mel([s for _, s in order], col0, stage, spec_min, spec_max)
        got: Dict[Tuple[int, int], Any] = {}
        i = 0
        while i < len(order):
            (t, bi, _), _ = order[i]
            j = i
            while j < len(order) and order[j][0][:2] == (t, bi):
                j += 1
            c = self._cfm_req[t]
            chunks, L = int(c["fold_in"][bi][0].shape[0]), lens[i]
            if j - i == chunks and bi not in c["mel"]:                  # the whole fold in this step: a column range of `stage`
                got[(t, bi)] = stage[:, col0[i]:col0[i] + chunks * L].unsqueeze(0)
            else:
                buf = c["mel"].setdefault(bi, [0, torch.empty(1, stage.shape[0], chunks * L, dtype=torch.float32, device=stage.device)])
                for n in range(i, j):
                    k = order[n][0][2]
                    buf[1][0, :, k * L:(k + 1) * L] = stage[:, col0[n]:col0[n] + L]
                buf[0] += j - i
                if buf[0] == chunks:
                    got[(t, bi)] = c["mel"].pop(bi)[1]
            i = j
        return got

    def _vocode(self, folds: List[Tuple[int, int]], staged: dict) -> None:
        """the completed folds through the vocoder -- one forward_segments pass (at most vocoder_max_frames frames each) when
        shared_vocoder, one call per fold otherwise -- and _fold_tail; a call that raises fails the requests of its folds"""
        import torch
        tts = self.tts
        calls: List[List[Tuple[int, int]]] = []
        frames = 0
        for f in folds:
            n = int(staged[f].shape[2])
            if not calls or not self._shared_vocoder or frames + n > int(tts.vocoder_max_frames):
                calls.append([])
                frames = 0
            calls[-1].append(f)
            frames += n
        for call in calls:
            try:
                mels = []
                for t, bi in call:
                    dt = self._cfm_req[t]["fold_in"][bi][0].dtype       # the dtype _fold_mel hands the vocoder in run_batch
                    mels.append(staged[(t, bi)].to(dt if dt in (torch.float16, torch.float32) else torch.float32).contiguous())
                if self._shared_vocoder:
                    audios = [a[0][0] for a in tts.vocoder.forward_segments(mels)]
                else:
                    audios = [tts.vocoder(m)[0][0] for m in mels]
                self._count(vocoder_calls=1 if self._shared_vocoder else len(mels))
                for (t, bi), m, audio in zip(call, mels, audios):
                    rows, lens, pad_len = self._cfm_req[t]["fold_in"][bi]
                    self._requests[t]["frags"][bi] = tts._fold_tail(audio, int(m.shape[2]) // int(rows.shape[0]), lens, pad_len)
            except Exception as e:                                      # noqa: BLE001 -- the folds of this vocoder call
                self._fail(sorted({t for t, _ in call}), e)

    def _fail(self, tickets: Iterable[int], exc: BaseException) -> None:
        """the requests get `exc` as their result; their rows, slots and buffers are dropped"""
        for t in tickets:
            if t in self._requests:
                self._forget(t)                     # a streaming request may still have rows in the decode session
                self._done.append((t, exc))

    def _drop_cfm(self, t: int) -> None:
        """forgets the request's flow-matching state: queued rows, live slots (released), fold buffers and, when no other
        request speaks with it, its voice's cached prompt features"""
        if self._cpol is None:
            return
        slots = self._cpol.cancel(t)
        if slots and self._cfm is not None:
            self._cfm.release(slots)
            self._count(cfm_released=len(slots))
            self.stats["events"].append(("cfm_release", slots))
        c = self._cfm_req.pop(t, None)
        if c is not None and all(o["vk"] != c["vk"] for o in self._cfm_req.values()):
            self._cfm_prompts.pop(c["vk"], None)

    def _close_cfm(self) -> None:
        if self._cfm is not None:
            try:
                self._cfm.close()
            finally:
                self._cfm = None

    def _close_sessions(self) -> None:
        if self._ses is not None:
            self._ses.close()
            self.sessions.append(self._ses)
            self._ses = None
        self._close_cfm()


_END = object()      # closes a Stream's queue


class Stream:
    """What `Server.submit_stream` returns: the iterator over one streaming request's fragments (see there)."""

    def __init__(self, server: "Server", future: concurrent.futures.Future):
        self._server, self.future = server, future
        self._over: Any = None

    def __iter__(self):
        return self

    def __next__(self):
        if self._over is None:
            item = self.future.fragments.get()
            if item is not _END and not isinstance(item, BaseException):
                return item
            self._over = item
        if self._over is _END:
            raise StopIteration
        raise self._over

    def cancel(self) -> None:
        """asks the server to cancel the request: the stream ends with CancelledError after the fragments already emitted"""
        self._server.cancel(self.future)


class Server:
    """One loop thread around a `Scheduler`: the only thread that touches the GPU.  `submit` works from any thread and returns
    a Future that resolves to the request's result (or raises its exception).  The loop sleeps on a condition variable while
    there is nothing to do.  An exception that escapes `Scheduler.step` fails every outstanding future with it and stops the
    loop; later `submit` calls raise."""

    def __init__(self, scheduler):
        self._sched = scheduler
        self._cv = threading.Condition()
        self._cmds: collections.deque = collections.deque()      # ("submit", request, future) | ("cancel", future)
        self._futures: Dict[int, concurrent.futures.Future] = {}
        self._stopping, self._drain, self._stopped = False, True, False
        self.error: Optional[BaseException] = None
        self._thread = threading.Thread(target=self._loop, name="gsv-serving", daemon=True)
        self._thread.start()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.shutdown()
        return False

    @property
    def scheduler(self):
        return self._sched

    def submit(self, request: dict) -> concurrent.futures.Future:
        fut: concurrent.futures.Future = concurrent.futures.Future()
        fut.fragments = queue.SimpleQueue()     # (sr, audio) as emitted, then _END or the exception: read by Stream
        with self._cv:
            if self.error is not None:
                raise RuntimeError(f"the server stopped: {self.error!r}") from self.error
            if self._stopping or self._stopped:
                raise RuntimeError("the server is shut down")
            self._cmds.append(("submit", request, fut))
            self._cv.notify_all()
        return fut

    def submit_stream(self, request: dict) -> "Stream":
        """a streaming request (`return_fragment` is set for it): an iterator over its fragments (sr, int16 audio) as the
        scheduler emits them.  `__next__` blocks until the next fragment is there and re-raises the request's exception
        (CancelledError after `cancel()`) once the fragments emitted before it are consumed; `.future` resolves to the list of
        all fragments."""
        stream = Stream(self, self.submit(dict(request, return_fragment=True)))
        return stream

    def cancel(self, future: concurrent.futures.Future) -> None:
        """asks the loop to cancel the request: its future raises CancelledError (unless it was delivered first)"""
        with self._cv:
            if not self._stopped:
                self._cmds.append(("cancel", None, future))
                self._cv.notify_all()

    def shutdown(self, drain: bool = True, timeout: Optional[float] = None) -> None:
        """stops the loop: after everything outstanding is delivered (drain=True), or at once, cancelling it"""
        with self._cv:
            self._stopping, self._drain = True, bool(drain)
            self._cv.notify_all()
        if threading.current_thread() is not self._thread:
            self._thread.join(timeout)

    def _deliver(self, results, fragments=()) -> None:
        for ticket, _, frag in fragments:
            fut = self._futures.get(ticket)
            if fut is not None:
                fut.fragments.put(frag)
        for ticket, result in results:
            fut = self._futures.pop(ticket, None)
            if fut is None:
                continue
            if isinstance(result, BaseException):
                fut.fragments.put(result)
                fut.set_exception(result)
            else:
                fut.fragments.put(_END)
                fut.set_result(result)

    def _loop(self) -> None:
        sched = self._sched
        try:
            while True:
                with self._cv:
                    while not self._cmds and not self._stopping and sched.idle:
                        self._cv.wait()
                    cmds = list(self._cmds)
                    self._cmds.clear()
                    if self._stopping and not cmds and (sched.idle or not self._drain):
                        break
                for kind, request, fut in cmds:
                    if kind == "submit":
                        if fut.set_running_or_notify_cancel():
                            try:
                                self._futures[sched.submit(request)] = fut
                            except Exception as e:           # noqa: BLE001 -- refused at the door: its own result, nobody else's
                                fut.fragments.put(e)
                                fut.set_exception(e)
                    else:
                        for ticket, f in list(self._futures.items()):
                            if f is fut:
                                sched.cancel(ticket)
                results = sched.step()
                take = getattr(sched, "take_fragments", None)
                self._deliver(results, take() if take is not None else ())
        except BaseException as e:                                      # noqa: BLE001 -- handed to every waiting future
            self.error = e
        finally:
            with self._cv:
                self._stopped = True
                left = [fut for kind, _, fut in self._cmds if kind == "submit" and fut.set_running_or_notify_cancel()]
                self._cmds.clear()
            left += list(self._futures.values())
            self._futures.clear()
            for fut in left:
                exc = self.error if self.error is not None else CancelledError()
                fut.fragments.put(exc)
                fut.set_exception(exc)
            try:
                sched.close()
            except Exception:                                           # noqa: BLE001 -- the loop is gone either way
                pass
