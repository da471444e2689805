"""Serving requests as they arrive: one open AR decode session, shared waveform passes.

`TTS.run_batch` takes a closed list and returns when the slowest request is done.  Here requests come in one by one:

* `Scheduler` is the core, single-threaded and deterministic.  `submit` only enqueues; every `step` takes in what was submitted,
  admits queued sentences into the free slots of ONE decode session (`T2SSession`, per-row keys and sampling values), advances
  the live rows a chunk of steps, and sends the requests whose sentences have all come back through the shared waveform stage
  of `run_batch` -- so a short request is delivered when it is finished, and a new one takes a free slot while the others
  decode.  A request that cannot decode in the session (prompt-free, `parallel_infer=False`, a row the K/V arena would cut,
  `return_fragment` / streaming, `best_of` candidates) is *exclusive*: a FIFO barrier that is served with `run_batch([request])` once nothing is live.
* `plan_online` is the schedule as a pure function, `plan_continuous` with arrivals: the event trace `Scheduler` records in
  `stats["events"]`.  Both are driven by the same `_Policy`, which holds every decision and touches no GPU.
* `Server` puts one loop thread around a scheduler: the only thread that makes GPU calls.  `submit` returns a
  `concurrent.futures.Future` from any thread.

What a request returns is what `run_batch([request])` returns for it alone: its rows carry the RNG keys and sampling tuples
`plan_batch` gives them, sampling is per row, admissions and releases leave the neighbouring slots untouched, and the waveform
stages are the ones `run_batch` pins against `run`.  AR launches and waveform passes are issued strictly one after the other
(DESIGN.md section 4o).
"""
from __future__ import annotations

import collections
import concurrent.futures
import threading
from concurrent.futures import CancelledError
from typing import Any, Dict, Iterable, List, Optional, Sequence, Tuple

from .AR.models.t2s_model import admit_count


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
        self.open = False          # a decode session is open
        self.dirty = False         # something ran since the last ("close",)

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
        return not self.fifo and not self.missing and not self.ready

    # -- one step, in the order Scheduler.step documents
    def arrive(self, req, rows: int, exclusive: bool, step: int) -> None:
        if exclusive:
            self.fifo.append([req, 0, 0, True])
        elif rows <= 0:
            self.ready.append((req, step))          # no sentence: nothing to decode
        else:
            self.fifo.append([req, int(rows), 0, False])
            self.missing[req] = int(rows)

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
            if self.missing[req] == 0:
                del self.missing[req]
                self.ready.append((req, step))

    def wave(self, step: int) -> list:
        """the requests of this step's waveform pass: all that are ready, once the oldest has waited wave_hold steps -- or at
        once when no row is live or admissible, since no company can come"""
        if not self.ready:
            return []
        if step - self.ready[0][1] < self.wave_hold and (self.live or self.queued):
            return []
        out = [req for req, _ in self.ready]
        self.ready = []
        self.dirty = True
        return out

    def exclusive_head(self):
        """the exclusive request to serve now, or None: it is the head of the queue and nothing is live"""
        if self.fifo and self.fifo[0][3] and not self.live:
            self.dirty = True
            return self.fifo.popleft()[0]
        return None

    def close_due(self) -> bool:
        """end of a step: nothing live, nothing queued -> the decoder is handed back (once per burst)"""
        if self.live or self.fifo or not self.dirty:
            return False
        self.open = self.dirty = False
        return True

    def cancel(self, req) -> List[int]:
        """forgets the request; returns the slots its live rows held"""
        for e in list(self.fifo):
            if e[0] == req:
                self.fifo.remove(e)
        self.missing.pop(req, None)
        self.ready = [(r, t) for r, t in self.ready if r != req]
        slots = [s for s, o in enumerate(self.owner) if o is not None and o[0] == req]
        for s in slots:
            self.owner[s] = None
        return slots


def plan_online(arrivals: Sequence[int], rows_per_request: Sequence[int], lengths: Sequence[int], slots: int, chunk: int,
                admit_min: Optional[int] = None, wave_hold: int = 0, exclusive=(), with_steps: bool = False):
    """The schedule `Scheduler` follows, as a pure function.  Request r is submitted in front of step arrivals[r] (requests
    arriving in the same step keep their order) and brings rows_per_request[r] rows; `lengths` lists, request after request and
    row after row, how many further steps each row needs after its step 0 (0: it ends at its admission), as `plan_continuous`
    takes them.  The requests named in `exclusive` bring no rows (their entry of rows_per_request is not read).  Returns the
    events ("admit", [(req, row, slot), ...]), ("advance", chunk, [(req, row) reported finished, in slot order]),
    ("wave", [reqs]), ("exclusive", req) and ("close",); with_steps=True, (step, event) pairs.  With every arrival at step 0 and
    no exclusive request the admit / advance events are `plan_continuous`'s."""
    n = len(arrivals)
    if len(rows_per_request) != n:
        raise ValueError(f"{len(rows_per_request)} row counts for {n} arrivals")
    excl = set(exclusive)
    first, total = {}, 0
    for r in range(n):
        first[r] = total
        total += 0 if r in excl else int(rows_per_request[r])
    if total != len(lengths):
        raise ValueError(f"{len(lengths)} lengths for {total} rows")
    pol = _Policy(slots, chunk, admit_min, wave_hold)
    order = sorted(range(n), key=lambda r: (int(arrivals[r]), r))
    left = [0] * pol.slots
    trace, nxt, step = [], 0, 0
    while nxt < n or not pol.idle:
        if pol.idle and int(arrivals[order[nxt]]) > step:
            step = int(arrivals[order[nxt]])            # nothing to do until the next arrival
        while nxt < n and int(arrivals[order[nxt]]) <= step:
            r = order[nxt]
            pol.arrive(r, 0 if r in excl else int(rows_per_request[r]), r in excl, step)
            nxt += 1
        admitted = pol.admit()
        if admitted:
            for r, row, s in admitted:
                left[s] = int(lengths[first[r] + row])
            trace.append((step, ("admit", admitted)))
        if pol.live:
            done = []
            for s in range(pol.slots):
                if pol.owner[s] is None:
                    continue
                left[s] -= min(pol.chunk, left[s])
                if left[s] == 0:
                    done.append(pol.owner[s])
            trace.append((step, ("advance", pol.chunk, done)))
            pol.finish(done, step)
        ready = pol.wave(step)
        if ready:
            trace.append((step, ("wave", ready)))
        while True:
            was_open = pol.open
            r = pol.exclusive_head()
            if r is None:
                break
            if was_open:
                pol.open = False
                trace.append((step, ("close",)))
            trace.append((step, ("exclusive", r)))
        if pol.close_due():
            trace.append((step, ("close",)))
        step += 1
    return trace if with_steps else [e for _, e in trace]


class Scheduler:
    """The step-driven scheduler over a loaded `TTS` pipeline.  Not thread-safe: one thread calls it (`Server`'s loop).
    slots: rows of the decode session (default: the decoder's max_batch); chunk: steps per advance; admit_min: as `admit_count`
    (default max(1, slots // 4)); wave_hold: steps a finished request may wait for others to share its waveform pass.
    shared_hubert / shared_bert / shared_sv / device_frontend / shared_vocoder: as `run_batch`'s keywords, applied to the
    requests one step takes in (front-ends) and to the requests one step finishes (vocoder)."""

    def __init__(self, tts, slots: Optional[int] = None, chunk: int = 32, admit_min: Optional[int] = None, wave_hold: int = 0,
                 shared_hubert: bool = True, shared_bert: bool = True, shared_sv: bool = False, device_frontend: bool = False,
                 shared_vocoder: bool = False):
        if tts.t2s_model is None or tts.vits_model is None:
            raise RuntimeError("init_t2s_weights / init_vits_weights first")
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
        self._inbox: List[Tuple[int, dict]] = []
        self._requests: Dict[int, dict] = {}        # ticket -> request (exclusive) or plan (session), until delivered
        self._rows: Dict[int, List[dict]] = {}      # ticket -> its rows in queue order: dict(bi, j, key, sampling)
        self._where: Dict[int, Tuple[int, int]] = {}    # session ticket -> (ticket, row)
        self._done: List[Tuple[int, Any]] = []      # results that wait for the next step to return them
        self._ses = None
        self._next, self._step = 0, 0
        self._closed = False
        self.sessions: list = []                    # every closed T2SSession, in order (history, modes, adopt times)
        self.stats: Dict[str, Any] = dict(steps=0, admissions=0, rows=0, advances=0, waves=0, exclusive=0, sessions=0, released=0,
                                          occupancy=[], events=[], tickets={})

    # -- public
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    @property
    def idle(self) -> bool:
        return not self._inbox and not self._done and self._pol.idle

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
        """drops the request's queued rows and releases its live ones; its result, returned by the next step, is
        CancelledError.  False if the ticket is not outstanding (unknown, or delivered)."""
        if any(t == ticket for t, _ in self._inbox):
            self._inbox = [(t, r) for t, r in self._inbox if t != ticket]
        elif ticket in self._requests:
            slots = self._pol.cancel(ticket)
            if slots:
                self._ses.release_slots(slots)
                self.stats["released"] += len(slots)
                self.stats["events"].append(("release", slots))
            self._where = {k: v for k, v in self._where.items() if v[0] != ticket}
            self._requests.pop(ticket)
            self._rows.pop(ticket, None)
        else:
            return False
        self._done.append((ticket, CancelledError()))
        return True

    def close(self) -> None:
        """drops what is outstanding (no step will return it) and closes the session: `tts.run` / `run_batch` work again"""
        for t in [t for t, _ in self._inbox] + list(self._requests):
            self.cancel(t)
        self._done = []
        self._close_session()
        self._closed = True

    def step(self) -> List[Tuple[int, Any]]:
        """One round: intake, admit, advance, finish, exclusive requests, close when idle (module docstring).  Returns the
        (ticket, result) pairs of the requests that ended in it; a result is (sr, int16 audio), the list of fragments of a
        `return_fragment` request, or the exception the request raised."""
        import torch
        with torch.no_grad():
            return self._do_step()

    # -- the step
    def _do_step(self) -> List[Tuple[int, Any]]:
        pol, step, ev = self._pol, self._step, self.stats["events"]
        out, self._done = self._done, []
        self._intake(out)
        admitted = pol.admit()
        if admitted:
            self._admit(admitted)
            ev.append(("admit", admitted))
        if pol.live:
            self.stats["occupancy"].append(pol.live)
            done = []
            for st, y, n in self._ses.advance(pol.chunk):
                t, row = self._where.pop(st)
                e = self._rows[t][row]
                pl = self._requests[t]
                pl["preds"][e["bi"]][e["j"]], pl["idxs"][e["bi"]][e["j"]] = y, n
                done.append((t, row))
            self.stats["advances"] += 1
            ev.append(("advance", pol.chunk, done))
            pol.finish(done, step)
        ready = pol.wave(step)
        if ready:
            ev.append(("wave", ready))
            self.stats["waves"] += 1
            self._wave(ready, out)
        while True:
            was_open = pol.open
            t = pol.exclusive_head()
            if t is None:
                break
            if was_open:
                pol.open = False
                self._close_session()
                ev.append(("close",))
            ev.append(("exclusive", t))
            self.stats["exclusive"] += 1
            self._exclusive(t, out)
        if pol.close_due():
            self._close_session()
            ev.append(("close",))
        for t, _ in out:
            self.stats["tickets"][t][2] = step
        self._step += 1
        self.stats["steps"] = self._step
        return out

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
        streaming = [(t, r) for t, r in taken if r.get("return_fragment") or r.get("streaming_mode")]
        plain = self._resolve([(t, r) for t, r in taken if not (r.get("return_fragment") or r.get("streaming_mode"))], out)
        plans = {}
        for t, req in plain:
            try:
                plans[t] = (req, self.tts._plan_request(req))
            except Exception as e:                                      # noqa: BLE001 -- the request's own result
                out.append((t, e))
        for t, req in sorted(streaming + [(t, rp[0]) for t, rp in plans.items()], key=lambda x: x[0]):    # arrival order
            rows = self._session_rows(plans[t][1]) if t in plans else None
            if rows is None:
                self._requests[t] = req
                self._pol.arrive(t, 0, True, self._step)
            else:
                pl = plans[t][1]
                pl["preds"] = [[None] * len(item["all_phones"]) for item in pl["data"]]
                pl["idxs"] = [[None] * len(item["all_phones"]) for item in pl["data"]]
                self._requests[t], self._rows[t] = pl, rows
                self._pol.arrive(t, len(rows), False, self._step)

    def _budget(self) -> int:
        from .TTS_infer_pack.TTS import early_stop_num
        return min(1500, int(early_stop_num(self.tts.configs)) + 1)

    def _session_rows(self, pl: dict) -> Optional[List[dict]]:
        """the request's rows in (bi, j) order with plan_batch's keys and sampling tuples -- or None: the request is exclusive
        (prompt-free, the naive loop, "best_of" candidates, or a row that does not fit the K/V arena with the full step budget)"""
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
                             prompt=pl["voice"]["prompt_semantic"].view(-1), key=e["key"], sampling=e["sampling"]))
            if self.stats["tickets"][t][1] is None:
                self.stats["tickets"][t][1] = self._step
        if self._ses is None:
            k, p, temp, rp = rows[0]["sampling"]        # placeholders: every row brings its own tuple
            self._ses = self.tts.t2s_model.open_session(self._pol.slots, k, p, temp, rp, early_stop_num(self.tts.configs), 1,
                                                        self._budget(), row_sampling=True)
            self.stats["sessions"] += 1
        tickets = self._ses.admit(rows, slots=[s for _, _, s in admitted])
        for st, (t, row, _) in zip(tickets, admitted):
            self._where[st] = (t, row)
        self.stats["admissions"] += 1
        self.stats["rows"] += len(rows)

    def _wave(self, ready: List[int], out: list) -> None:
        """the ready requests through run_batch's waveform stages, called with the ready subset, then each through
        _finish_request; a stage that raises fails the requests of this pass, nobody else"""
        tts = self.tts
        plans = [self._requests.pop(t) for t in ready]
        for t in ready:
            self._rows.pop(t, None)
        try:
            for pl in plans:
                pl["kept"] = [tts._kept_tokens(p, i, pl["no_prompt"]) for p, i in zip(pl["preds"], pl["idxs"])]
            tts._wait_stream()
            sr = tts._output_sr()
            if tts.configs.use_vocoder:
                tts._shared_cfm_stage(plans, shared_vocoder=self._shared_vocoder)
            else:
                tts._shared_sovits_stage(plans)
        except Exception as e:                                          # noqa: BLE001 -- the pass's requests' result
            out.extend((t, e) for t in ready)
            return
        for t, pl in zip(ready, plans):
            try:
                out.append((t, tts._finish_request(pl, sr)))
            except Exception as e:                                      # noqa: BLE001 -- the request's own result
                out.append((t, e))

    def _exclusive(self, t: int, out: list) -> None:
        req = self._requests.pop(t)
        try:
            if req.get("return_fragment") or req.get("streaming_mode"):
                out.append((t, list(self.tts.run(dict(req, return_fragment=True)))))
            else:
                out.append((t, self.tts.run_batch([req])[0]))
        except Exception as e:                                          # noqa: BLE001 -- the request's own result
            out.append((t, e))

    def _close_session(self) -> None:
        if self._ses is not None:
            self._ses.close()
            self.sessions.append(self._ses)
            self._ses = None
        self._pol.open = False


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
        with self._cv:
            if self.error is not None:
                raise RuntimeError(f"the server stopped: {self.error!r}") from self.error
            if self._stopping or self._stopped:
                raise RuntimeError("the server is shut down")
            self._cmds.append(("submit", request, fut))
            self._cv.notify_all()
        return fut

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

    def _deliver(self, results) -> None:
        for ticket, result in results:
            fut = self._futures.pop(ticket, None)
            if fut is None:
                continue
            if isinstance(result, BaseException):
                fut.set_exception(result)
            else:
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
                            self._futures[sched.submit(request)] = fut
                    else:
                        for ticket, f in list(self._futures.items()):
                            if f is fut:
                                sched.cancel(ticket)
                self._deliver(sched.step())
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
                fut.set_exception(self.error if self.error is not None else CancelledError())
            try:
                sched.close()
            except Exception:                                           # noqa: BLE001 -- the loop is gone either way
                pass
