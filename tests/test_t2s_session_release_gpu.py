"""GPU: gsv_t2s_session_release / T2SSession.release -- rows taken out of an open decode session (a cancelled request) on the
small fp32 decoder of test_t2s_session_gpu.py, 4 slots: the released slots stop, their neighbours decode what they decode
uninterrupted and keep the K/V they had, the slots are admitted again, and a refused release changes nothing."""
import numpy as np
import pytest
import torch

from oracle import cases
from test_t2s_ragged_gpu import DEV, _dev, _engine, _rows
from test_t2s_session_gpu import QUEUE_SEED, _kv_of, _session_rows

pytestmark = pytest.mark.gpu

KW = dict(top_k=15, top_p=1.0, temperature=1.0, early_stop_num=40, repetition_penalty=1.35)


@pytest.fixture(scope="module")
def setup():
    """the decoder, 6 session rows and the tokens each decodes alone with its key"""
    cfg, sd, *_ = cases.t2s_case_inputs(cases.T2S_CASES["t2s_small_greedy"])
    eng = _engine(cfg, sd, torch.float32, max_batch=8, max_seq=320)
    xs, berts, prompts = _rows(cfg, 6, seed=QUEUE_SEED, zh_bert=True)
    xd, bd = _dev(xs, berts)
    pd = [p.to(DEV) for p in prompts]
    keys = [(3000 + 13 * b, (3 * b + 1) % 5) for b in range(6)]
    alone = []
    for b in range(6):
        y, i = eng.infer_panel_batch_infer([xd[b]], None, [pd[b]], [bd[b]], rng_keys=[keys[b]], **KW)
        alone.append((y[0].tolist(), i[0]))
    assert min(i for _, i in alone[:4]) > 8, "the first four rows must still be decoding after two chunks of 4"
    return eng, _session_rows(xd, bd, pd, keys), alone


def _drain(ses, chunk=16):
    done = {}
    calls = 0
    while ses.live:
        for t, y, n in ses.advance(chunk):
            done[t] = (y.tolist(), n)
        calls += 1
        assert calls <= 20
    return done


def test_released_rows_stop_neighbours_go_on_and_the_slots_are_admitted_again(setup):
    eng, rows, alone = setup
    with eng.open_session(4, **KW) as ses:
        assert ses.admit(rows[:4]) == [0, 1, 2, 3]
        assert ses.advance(4) == []
        st0 = ses.state()
        assert st0[1].tolist() == [1, 1, 1, 1] and st0[2].tolist() == [5, 5, 5, 5]
        kv0 = {s: _kv_of(eng, s, int(st0[0][s])) for s in (0, 2)}
        assert ses.release([1, 3, 99]) == [1, 3], "a ticket that holds no slot is skipped"
        st1 = ses.state()
        assert st1[1].tolist() == [1, 0, 1, 0], "state() shows the released rows not live"
        assert ses.free == [1, 3] and ses.live == 2
        assert np.array_equal(st1[[0, 2, 3]], st0[[0, 2, 3]]), "a release touches the live words only"
        assert ses.advance(4) == []
        st2 = ses.state()
        assert st2[2].tolist() == [9, 5, 9, 5] and st2[0, 1] == st0[0, 1] and st2[0, 3] == st0[0, 3], \
            "the released rows' step counters and caches stop"
        done = _drain(ses)
        assert sorted(done) == [0, 2], "no advance reports a released row"
        for t in (0, 2):
            assert done[t] == alone[t], f"row {t} decodes other tokens after its neighbours were released"
            assert all(torch.equal(a, b) for a, b in zip(kv0[t], _kv_of(eng, t, int(st0[0][t])))), \
                f"slot {t}: K/V written before the release changed"
        # the released slots take new rows, which decode what they decode alone
        assert ses.release([1, 3]) == [] and ses.free == [0, 1, 2, 3]
        assert ses.admit(rows[4:6], slots=[1, 3]) == [4, 5]
        assert ses.state()[1].tolist() == [0, 1, 0, 1]
        done = _drain(ses)
        assert sorted(done) == [4, 5]
        for t in (4, 5):
            assert done[t] == alone[t], f"row {t} decodes other tokens in a released slot"
        assert ses.history == [(0, 0), (1, 1), (2, 2), (3, 3), (4, 1), (5, 3)]


def test_a_refused_release_changes_nothing(setup):
    eng, rows, alone = setup
    with eng.open_session(4, **KW) as ses:
        ses.admit(rows[:3])
        assert ses.advance(4) == []
        st0 = ses.state()
        for bad in ([4], [-1], [0, 7], [2, 2], [0, 1, 0]):
            with pytest.raises(RuntimeError, match=r"rc=-1"):
                ses.release_slots(bad)
            assert np.array_equal(ses.state(), st0) and ses.live == 3 and ses.free == [3]
        # a slot that holds no live row is left as it is
        assert ses.release_slots([3]) == [3] and np.array_equal(ses.state(), st0)
        done = _drain(ses)                           # the session goes on as if nothing had been refused
        assert {t: done[t] for t in range(3)} == {t: alone[t] for t in range(3)}
    with pytest.raises(RuntimeError, match=r"rc=-3"):
        ses.release_slots([0])                       # no session open
    # ... and the handle is as usable as after any closed session
    with eng.open_session(4, **KW) as ses:
        ses.admit(rows[:1])
        assert _drain(ses)[0] == alone[0]
