"""CPU: gsv.serving.Server over a fake scheduler that does no GPU work (futures, errors, shutdown; every wait has a timeout),
tts_handle with and without a server, and the ABI of gsv_t2s_session_release."""
import os
import re
import threading
from concurrent.futures import CancelledError

import pytest

from conftest import ROOT
from gsv import wire
from gsv.serving import Server

WAIT = 20.0      # seconds: far above anything these tests take; a bug fails instead of hanging


class FakeScheduler:
    """the Scheduler interface Server uses; a request {"n": k} is delivered by the k-th step after its intake as ("done", its
    payload) -- or, with "raise", as that exception; "boom" makes step() itself raise"""

    def __init__(self):
        self.inbox, self.work, self.done, self.next = [], {}, [], 0
        self.threads, self.steps, self.closed = set(), 0, False

    @property
    def idle(self):
        return not self.inbox and not self.work and not self.done

    def submit(self, request):
        self.threads.add(threading.get_ident())
        t, self.next = self.next, self.next + 1
        self.inbox.append((t, request))
        return t

    def cancel(self, ticket):
        self.threads.add(threading.get_ident())
        self.inbox = [(t, r) for t, r in self.inbox if t != ticket]
        self.work.pop(ticket, None)
        self.done.append((ticket, CancelledError()))
        return True

    def step(self):
        self.threads.add(threading.get_ident())
        self.steps += 1
        for t, r in self.inbox:
            self.work[t] = [int(r.get("n", 1)), r]
        self.inbox = []
        out, self.done = self.done, []
        for t in sorted(self.work):
            left, r = self.work[t]
            if r.get("boom"):
                raise RuntimeError("the engine fell over")
            if left <= 1:
                del self.work[t]
                out.append((t, r["raise"] if "raise" in r else ("done", r.get("payload"))))
            else:
                self.work[t][0] = left - 1
        return out

    def close(self):
        self.closed = True


def test_futures_resolve_to_their_own_results_from_several_threads():
    sched = FakeScheduler()
    server = Server(sched)
    got, errors = {}, []

    def client(c):
        try:
            futs = [(k, server.submit({"n": 1 + (c + k) % 4, "payload": (c, k)})) for k in range(8)]
            for k, f in futs:
                got[(c, k)] = f.result(timeout=WAIT)
        except Exception as e:                       # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=client, args=(c,)) for c in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(WAIT)
    assert not any(t.is_alive() for t in threads) and not errors
    assert got == {(c, k): ("done", (c, k)) for c in range(4) for k in range(8)}
    server.shutdown(timeout=WAIT)
    assert sched.closed and len(sched.threads) == 1 and threading.get_ident() not in sched.threads, \
        "only the loop thread may call the scheduler"


def test_the_loop_sleeps_when_idle():
    sched = FakeScheduler()
    server = Server(sched)
    assert server.submit({"n": 2}).result(timeout=WAIT) == ("done", None)
    assert server.submit({"n": 1}).result(timeout=WAIT) == ("done", None)
    server.shutdown(timeout=WAIT)
    # two steps for the first request, one for the second, none while idle or at shutdown: a loop that spins makes more
    assert sched.steps == 3, "an idle server must not step"


def test_a_requests_exception_lands_in_its_own_future_only():
    with Server(FakeScheduler()) as server:
        a = server.submit({"n": 2, "payload": "a"})
        b = server.submit({"n": 1, "raise": ValueError("bad reference")})
        c = server.submit({"n": 3, "payload": "c"})
        with pytest.raises(ValueError, match="bad reference"):
            b.result(timeout=WAIT)
        assert a.result(timeout=WAIT) == ("done", "a") and c.result(timeout=WAIT) == ("done", "c")


def test_cancel_resolves_the_future_with_cancelled_error():
    with Server(FakeScheduler()) as server:
        a = server.submit({"n": 10 ** 9, "payload": "a"})
        b = server.submit({"n": 2, "payload": "b"})
        server.cancel(a)
        with pytest.raises(CancelledError):
            a.result(timeout=WAIT)
        assert b.result(timeout=WAIT) == ("done", "b")


def test_an_exception_escaping_step_fails_every_pending_future_and_later_submits_raise():
    sched = FakeScheduler()
    server = Server(sched)
    ok = server.submit({"n": 1, "payload": "first"})
    assert ok.result(timeout=WAIT) == ("done", "first")
    pending = [server.submit({"n": 10 ** 9}) for _ in range(3)]
    bad = server.submit({"boom": True})
    for f in pending + [bad]:
        with pytest.raises(RuntimeError, match="fell over"):
            f.result(timeout=WAIT)
    server.shutdown(timeout=WAIT)           # the loop has stopped by itself
    assert not server._thread.is_alive() and sched.closed
    with pytest.raises(RuntimeError, match="stopped"):
        server.submit({"n": 1})


def test_shutdown_drain_delivers_everything_and_no_drain_cancels():
    server = Server(FakeScheduler())
    futs = [server.submit({"n": 1 + k % 5, "payload": k}) for k in range(20)]
    server.shutdown(drain=True, timeout=WAIT)
    assert not server._thread.is_alive()
    assert [f.result(timeout=0) for f in futs] == [("done", k) for k in range(20)]
    with pytest.raises(RuntimeError, match="shut down"):
        server.submit({"n": 1})
    server = Server(FakeScheduler())
    futs = [server.submit({"n": 10 ** 9}) for _ in range(4)]
    server.shutdown(drain=False, timeout=WAIT)
    assert not server._thread.is_alive()
    for f in futs:
        assert f.done(), "no future may be left pending"
        with pytest.raises(CancelledError):
            f.result(timeout=0)


# ---- the wire seam

class FakePipeline:
    def __init__(self):
        self.ran = []

    def run(self, req):
        import numpy as np
        self.ran.append(req)
        yield 32000, np.arange(8, dtype=np.int16)


class FakeServer:
    def __init__(self, result):
        self.result, self.submitted = result, []

    def submit(self, req):
        from concurrent.futures import Future
        self.submitted.append(req)
        f = Future()
        if isinstance(self.result, BaseException):
            f.set_exception(self.result)
        else:
            f.set_result(self.result)
        return f


def test_tts_handle_without_a_server_calls_run_as_before():
    pipe = FakePipeline()
    code, mt, payload = wire.tts_handle(pipe, {"text": "x", "media_type": "raw"})
    assert (code, mt) == (200, "audio/raw") and len(payload) == 16 and pipe.ran == [{"text": "x", "media_type": "raw"}]


def test_tts_handle_routes_through_the_server():
    import numpy as np
    pipe = FakePipeline()
    audio = np.arange(10, 22, dtype=np.int16)
    server = FakeServer((32000, audio))
    code, mt, payload = wire.tts_handle(pipe, {"text": "x", "media_type": "raw"}, server=server)
    assert (code, mt) == (200, "audio/raw") and payload == audio.tobytes()
    assert pipe.ran == [] and server.submitted == [{"text": "x", "media_type": "raw"}]
    # streaming: an exclusive request whose fragments come back as a list and are framed here
    server = FakeServer([(32000, audio[:4]), (32000, audio[4:])])
    code, mt, payload = wire.tts_handle(pipe, {"text": "x", "media_type": "raw", "streaming_mode": True}, server=server)
    assert code == 200 and b"".join(payload) == audio.tobytes()
    assert pipe.ran == [] and server.submitted[0]["return_fragment"] is True
    # a failed request answers 400 with the message, as without a server
    code, mt, payload = wire.tts_handle(pipe, {"text": "x"}, server=FakeServer(ValueError("no such voice")))
    assert code == 400 and payload == {"message": "tts failed", "Exception": "no such voice"}


def test_create_app_routes_tts_through_the_server_and_without_one_through_run():
    pytest.importorskip("fastapi")
    pytest.importorskip("httpx")
    import numpy as np
    from fastapi.testclient import TestClient

    class AudioScheduler(FakeScheduler):
        def step(self):
            return [(t, r if isinstance(r, BaseException) else (32000, np.arange(4, dtype=np.int16))) for t, r in super().step()]
    pipe = FakePipeline()
    client = TestClient(wire.create_app(pipe))
    r = client.post("/tts", json={"text": "x", "media_type": "raw"})
    assert r.status_code == 200 and len(r.content) == 16 and len(pipe.ran) == 1
    r = client.get("/tts", params={"text": "x", "media_type": "raw", "top_k": "3"})
    assert r.status_code == 200 and pipe.ran[-1] == {"text": "x", "media_type": "raw", "top_k": 3}
    with Server(AudioScheduler()) as server:
        client = TestClient(wire.create_app(pipe, server=server))
        r = client.post("/tts", json={"text": "x", "media_type": "raw", "n": 3})
        assert r.status_code == 200 and r.content == np.arange(4, dtype=np.int16).tobytes() and len(pipe.ran) == 2
    assert server.scheduler.steps == 3 and server.scheduler.closed


# ---- ABI

def test_the_header_declares_and_the_library_binds_session_release():
    from gsv import _lib, build
    src = open(os.path.join(ROOT, "include", "gsv.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+gsv_t2s_session_release\s*\(\s*gsv_t2s_t\s*\*\s*h\s*,\s*int\s+n\s*,\s*const\s+int32_t\s*\*\s*slot_ids\s*,"
                     r"\s*gsv_stream_t\s+stream\s*\)\s*;", src)
    assert "gsv_t2s_session_release" in _lib.EXPORTS
    build.build(verbose=False)
    l = _lib.lib()
    assert hasattr(l, "gsv_t2s_session_release") and len(l.gsv_t2s_session_release.argtypes) == 4
    assert l.gsv_abi_version() == 1
