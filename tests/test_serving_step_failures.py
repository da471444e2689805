"""CPU: gsv.serving._run_step, the step `Scheduler` and `plan_online` share, under a backend whose stages raise.  The backend
is `plan_online`'s own (`_Replay`) with one stage that throws an ordinary RuntimeError when asked to, and with the bookkeeping
of `Scheduler._fail`: a failed request gets the exception as its result and leaves both policies through `cancel`.  No GPU
and no pipeline.  Every case is written out by hand: 4 decode slots, chunk 8, every AR row done at its admission, so step 0
admits and finishes all rows; cfm_chunk 2.  Checked: who gets the exception, that every other request is served with the
events it has without the failed ones, that both policies end idle behind one close, and that the next burst starts a fresh
session in slot 0."""
from gsv.serving import _CfmPolicy, _Policy, _Replay, _run_step

U = False
BOOM = RuntimeError("boom")


class _Failing(_Replay):
    def __init__(self, pol, cp, cfm_folds, stage=None, when=None):
        super().__init__(pol.slots, [0] * 8, dict.fromkeys(cfm_folds, 0), cfm_folds)     # every row needs 0 further steps
        self.pol, self.cp, self.results = pol, cp, {}
        if stage is not None:
            inner = getattr(self, stage)

            def failing(*args):
                if when(*args):
                    raise BOOM
                return inner(*args)
            setattr(self, stage, failing)

    def _fail(self, reqs, exc):
        for r in reqs:
            if r not in self.results:
                self.pol.cancel(r)
                if self.cp is not None:
                    self.cp.cancel(r)
                self.results[r] = exc

    def _emit(self, due, ends):
        self.results.update({r: "fragments" for r in ends})
        return due

    def _deliver(self, reqs):
        reqs = [r for r in reqs if r not in self.results]
        self.results.update({r: "audio" for r in reqs})
        return reqs


def _serve(cfm_folds, cfm_rows=4, streaming=(), **fail):
    """the requests {r: their flow-matching rows per fold} arrive together; a streaming one has one AR row per fold, the
    others one.  cfm_rows=None: no flow-matching session.  Steps until idle -> (events, results), and the same again for a
    next burst of one request 9 on the same policies"""
    pol, cp = _Policy(4, 8, 1, 0), None if cfm_rows is None else _CfmPolicy(cfm_rows, 2)
    out = []
    for step0, burst, kw in ((0, cfm_folds, fail), (100, {9: [[(2, U)]]}, {})):
        assert pol.idle and not pol.open and (cp is None or not (cp.busy or cp.open or cp.pending or cp.folds))
        be = _Failing(pol, cp, burst, **kw)
        for r, f in burst.items():
            pol.arrive(r, len(f) if r in streaming else 1, False, step0, [1] * len(f) if r in streaming else None)
        ev, step = [], step0
        while not pol.idle or (cp is not None and cp.busy):
            _run_step(pol, cp, be, step, ev)
            step += 1
            assert step < step0 + 20
        out += [ev, be.results]
    return out


AR3 = [("admit", [(0, 0, 0), (1, 0, 1), (2, 0, 2)]), ("advance", 8, [(0, 0), (1, 0), (2, 0)])]
NEXT = [("admit", [(9, 0, 0)]), ("advance", 8, [(9, 0)]), ("cfm_admit", [(9, 0, 0, 0)]), ("cfm_step", 2, [(9, 0, 0)]),
        ("vocode", [(9, 0)]), ("deliver", [9]), ("close",)]


def test_encode_fails_the_request_it_encodes():
    one = [[(2, U)]]
    ev, results, ev2, results2 = _serve({0: one, 1: one, 2: one}, stage="_encode", when=lambda r, bi: r == 1)
    assert results == {0: "audio", 1: BOOM, 2: "audio"}
    # the others are served as if request 1 had never been encoded: none of its rows reaches the session
    assert ev == AR3 + [("cfm_admit", [(0, 0, 0, 0), (2, 0, 0, 1)]), ("cfm_step", 2, [(0, 0, 0), (2, 0, 0)]),
                        ("vocode", [(0, 0), (2, 0)]), ("deliver", [0, 2]), ("close",)]
    assert ev2 == NEXT and results2 == {9: "audio"}


def test_cfm_admit_fails_the_requests_of_that_admission():
    one = [[(2, U)]]
    # two DiT rows: requests 0 and 1 are the first admission, request 2 waits in the FIFO
    ev, results, ev2, results2 = _serve({0: one, 1: one, 2: one}, cfm_rows=2, stage="_cfm_admit", when=lambda a: a[0][0] == 0)
    assert results == {0: BOOM, 1: BOOM, 2: "audio"}
    assert ev == AR3 + [("cfm_admit", [(0, 0, 0, 0), (1, 0, 0, 1)]),                     # step 0: fails; nothing is live
                        ("cfm_admit", [(2, 0, 0, 0)]), ("cfm_step", 2, [(2, 0, 0)]),     # step 1: the slots are free again
                        ("vocode", [(2, 0)]), ("deliver", [2]), ("close",)]
    assert ev2 == NEXT and results2 == {9: "audio"}


def test_cfm_step_fails_every_request_with_a_live_row_and_queued_rows_open_the_next_session():
    ev, results, ev2, results2 = _serve({0: [[(4, U)]], 1: [[(2, U)]], 2: [[(2, U)]]}, cfm_rows=2, stage="_cfm_step",
                                        when=lambda k, done: done == [((1, 0, 0), 1)])
    # request 0 had two of its four Euler steps, request 1 was finished by the step that raised: both held a row
    assert results == {0: BOOM, 1: BOOM, 2: "audio"}
    assert ev == AR3 + [("cfm_admit", [(0, 0, 0, 0), (1, 0, 0, 1)]), ("cfm_step", 2, [(1, 0, 0)]),       # no vocode of (1, 0)
                        ("cfm_admit", [(2, 0, 0, 0)]), ("cfm_step", 2, [(2, 0, 0)]), ("vocode", [(2, 0)]), ("deliver", [2]),
                        ("close",)]
    assert ev2 == NEXT and results2 == {9: "audio"}


def test_vocode_fails_the_requests_of_that_call():
    ev, results, ev2, results2 = _serve({0: [[(2, U)]], 1: [[(4, U)]], 2: [[(2, U)]]}, stage="_vocode",
                                        when=lambda folds, mels: folds == [(0, 0), (2, 0)])
    assert results == {0: BOOM, 1: "audio", 2: BOOM}
    assert ev == AR3 + [("cfm_admit", [(0, 0, 0, 0), (1, 0, 0, 1), (2, 0, 0, 2)]), ("cfm_step", 2, [(0, 0, 0), (2, 0, 0)]),
                        ("vocode", [(0, 0), (2, 0)]),                                    # fails: nobody is delivered in step 0
                        ("cfm_step", 2, [(1, 0, 0)]), ("vocode", [(1, 0)]), ("deliver", [1]), ("close",)]
    assert ev2 == NEXT and results2 == {9: "audio"}


def test_emit_fails_the_requests_of_that_call():
    folds = {0: [[(2, U)]], 1: [[(2, U)], [(2, U)]]}                  # request 1 streams its two folds
    ar = [("admit", [(0, 0, 0), (1, 0, 1), (1, 1, 2)]), ("advance", 8, [(0, 0), (1, 0), (1, 1)])]
    ev, results, ev2, results2 = _serve(folds, streaming=[1], stage="_emit", when=lambda due, ends: ends == [1])
    assert results == {0: "audio", 1: BOOM}
    assert ev == ar + [("cfm_admit", [(0, 0, 0, 0), (1, 0, 0, 1), (1, 1, 0, 2)]), ("cfm_step", 2, [(0, 0, 0), (1, 0, 0), (1, 1, 0)]),
                       ("vocode", [(0, 0), (1, 0), (1, 1)]), ("deliver", [0]), ("close",)]       # and no fragment
    assert ev2 == NEXT and results2 == {9: "audio"}
    # without the flow-matching session the folds ride in request 0's waveform pass; request 0 is delivered before they fail
    ev, results, ev2, results2 = _serve(folds, cfm_rows=None, streaming=[1], stage="_emit", when=lambda due, ends: True)
    assert results == {0: "audio", 1: BOOM}
    assert ev == ar + [("wave", [0], [(1, 0), (1, 1)]), ("close",)]
    assert ev2 == [("admit", [(9, 0, 0)]), ("advance", 8, [(9, 0)]), ("wave", [9]), ("close",)] and results2 == {9: "audio"}


def test_the_waveform_pass_fails_its_requests_and_its_streams():
    folds = {0: [[(2, U)]], 1: [[(2, U)], [(2, U)]]}
    ev, results, ev2, results2 = _serve(folds, cfm_rows=None, streaming=[1], stage="_wave", when=lambda ready, sfolds: True)
    assert results == {0: BOOM, 1: BOOM}
    assert ev[2:] == [("wave", [0], [(1, 0), (1, 1)]), ("close",)]
    assert ev2[-2:] == [("wave", [9]), ("close",)] and results2 == {9: "audio"}


def test_without_a_failure_fragments_come_in_fold_order_and_end_the_request():
    ev, results, _, _ = _serve({0: [[(2, U)]], 1: [[(2, U)], [(2, U)]]}, streaming=[1])
    assert results == {0: "audio", 1: "fragments"}
    assert ev[-4:] == [("fragment", 1, 0), ("fragment", 1, 1), ("deliver", [0]), ("close",)]
