"""GPU: gsv_cfm_session_fetch_mel (CFMSession.fetch_mel) -- finished session rows in one launch, de-normalised and channels-first,
at their columns of the packed mel the vocoder reads.  The yardstick is the path it replaces, run from identical admissions:
fetch(slot), the slice behind the prompt frames, TTS.denorm_spec.  Both are fp32 and the arithmetic is the same expression in
the same order, so the bar is bit-equality."""
import ctypes as C

import pytest
import torch

from gsv.TTS_infer_pack.TTS import denorm_spec, spec_max, spec_min
from test_cfm_rows_gpu import DEV, _cfm, _rows, _small

pytestmark = pytest.mark.gpu
SENTINEL = -777.0


def _finished(cfm, T, tps, steps, tag, cap=None):
    """an open session whose rows (prompt lengths tps, step counts steps) were admitted into slots 0 .. n-1 and stepped to the end"""
    cfg = _small()[0]
    mu, prompts, noise = _rows(cfg, T, list(tps), tag)
    sess = cfm.open_session(cap or len(tps), T)
    slots = sess.admit(mu.to(DEV), [p.to(DEV) for p in prompts], list(steps), 0.0, noise=noise)
    assert slots == list(range(len(tps)))
    sess.step(max(steps))
    assert all(st[0] == sess.FINISHED for st in sess.state[:len(tps)])
    return sess


def _per_slot(cfm, T, tps, steps, tag):
    """the path fetch_mel replaces: per slot one fetch, the slice behind the prompt, denorm_spec"""
    with _finished(cfm, T, tps, steps, tag) as sess:
        return [denorm_spec(sess.fetch(s)[:, tp:]) for s, tp in enumerate(tps)]


def _columns(tps, T, gap, descending):
    """col0 per row: the ranges back to back with `gap` columns between them (and in front), laid out in descending row order
    when asked; -> (col0, ld)"""
    order = list(range(len(tps)))[::-1] if descending else list(range(len(tps)))
    col0, pos = [0] * len(tps), gap
    for b in order:
        col0[b] = pos
        pos += T - tps[b] + gap
    return col0, pos


def _check(cfm, T, tps, steps, tag, gap=3, descending=True):
    md = _small()[0]["mel_dim"]
    want = _per_slot(cfm, T, tps, steps, tag)
    col0, ld = _columns(tps, T, gap, descending)
    out = torch.full((md, ld), SENTINEL, device=DEV)
    with _finished(cfm, T, tps, steps, tag) as sess:
        assert sess.fetch_mel(list(range(len(tps))), col0, out, spec_min, spec_max) is out
        assert all(st == (sess.FREE, 0, 0) for st in sess.state)
    touched = torch.zeros(ld, dtype=torch.bool, device=DEV)
    for b, tp in enumerate(tps):
        got = out[:, col0[b]:col0[b] + T - tp]
        assert torch.isfinite(got).all() and torch.equal(got, want[b]), f"row {b} (Tp = {tp}) differs from fetch + denorm_spec"
        touched[col0[b]:col0[b] + T - tp] = True
    assert touched.sum().item() == sum(T - tp for tp in tps) < ld
    assert bool((out[:, ~touched] == SENTINEL).all()), "a column outside the ranges was written"
    assert not bool((out[:, touched] == SENTINEL).any())


@pytest.fixture(scope="module")
def cfm():
    cfg, sd, _, _, _ = _small()
    return _cfm(cfg, sd, torch.float32)


def test_rows_of_every_prompt_length_are_bit_equal_to_fetch_and_denorm(cfm):
    """T = 40 (smaller than the 64-frame tile): Tp = 0, T - 1, two in between and T (no generated frame: nothing written), with
    their own step counts, descending col0 with gaps.  n = rows_cap."""
    _check(cfm, 40, [0, 39, 17, 5, 40], [2, 1, 3, 2, 1], "mel40")


def test_a_length_that_is_no_multiple_of_the_tile_in_either_direction(cfm):
    """T = 150, mel = 100: 2 full + 1 partial frame tile, 1 full + 1 partial channel tile; lengths 150, 149, 86 (crosses a tile
    boundary at an odd offset), 64 (exactly one tile), 65 and 1.  Ascending col0 without gaps as well."""
    tps = [0, 1, 64, 86, 85, 149]
    _check(cfm, 150, tps, [1, 2, 1, 1, 2, 1], "mel150")
    _check(cfm, 150, tps, [1, 2, 1, 1, 2, 1], "mel150", gap=0 + 1, descending=False)


def test_one_row_of_a_larger_session(cfm):
    """n = 1 out of four finished slots: slot 2 goes (FREE), the others stay FINISHED and give later what an undisturbed
    session gives; slot 2 is admitted into again and its new row is the row of a fresh session"""
    T, tps, steps = 40, [3, 0, 11, 39], [2, 2, 3, 1]
    md = _small()[0]["mel_dim"]
    want = _per_slot(cfm, T, tps, steps, "one")
    cfg = _small()[0]
    mu, prompts, noise = _rows(cfg, T, [7], "again")
    with cfm.open_session(1, T) as fresh:
        s = fresh.admit(mu.to(DEV), [prompts[0].to(DEV)], 2, 0.0, noise=noise)[0]
        fresh.step(2)
        want_again = denorm_spec(fresh.fetch(s)[:, 7:])
    out = torch.full((1, md, 64), SENTINEL, device=DEV)             # the [1, mel, ld] form the vocoder takes
    with _finished(cfm, T, tps, steps, "one") as sess:
        sess.fetch_mel([2], [20], out, spec_min, spec_max)
        assert [st[0] for st in sess.state] == [sess.FINISHED, sess.FINISHED, sess.FREE, sess.FINISHED]
        assert torch.equal(out[0, :, 20:20 + T - 11], want[2])
        assert bool((out[0, :, :20] == SENTINEL).all()) and bool((out[0, :, 20 + T - 11:] == SENTINEL).all())
        assert sess.admit(mu.to(DEV), [prompts[0].to(DEV)], 2, 0.0, noise=noise) == [2]
        assert sess.step(2) == [2]
        for b in (0, 1, 3):
            assert torch.equal(denorm_spec(sess.fetch(b)[:, tps[b]:]), want[b])
        out2 = torch.full((md, T - 7), SENTINEL, device=DEV)
        sess.fetch_mel([2], [0], out2, spec_min, spec_max)
        assert torch.equal(out2, want_again)


def _raw(cfm, slots, col0, ld, out, n=None, null=None):
    from gsv import _lib
    dit = cfm.estimator
    k = len(slots)
    a = None if null == "slots" else (C.c_int32 * max(1, k))(*slots)
    b = None if null == "col0" else (C.c_int * max(1, k))(*col0)
    rc = _lib.lib().gsv_cfm_session_fetch_mel(dit._h, k if n is None else n, a, b, ld, float(spec_min), float(spec_max),
                                              None if null == "out" else out.data_ptr(), C.c_void_p(dit.stream.cuda_stream))
    dit.stream.synchronize()
    return rc


def test_refusals_leave_every_slot_and_every_byte_as_they_were(cfm):
    """a live slot, a free slot, a slot out of range, a repeated slot, n = 0 and n = rows_cap + 1, null slots / col0 / out,
    col0 < 0, a range one column past ld: each returns an error; the states stay, `out` keeps its sentinel, and the rows then
    come out with the bits of an undisturbed session"""
    T, md = 40, _small()[0]["mel_dim"]
    cfg = _small()[0]
    tps, steps = [4, 0, 9], [1, 1, 3]
    want = _per_slot(cfm, T, tps, steps, "refuse")[:2]
    mu, prompts, noise = _rows(cfg, T, tps, "refuse")
    ld = 100
    out = torch.full((md, ld), SENTINEL, device=DEV)
    with cfm.open_session(4, T) as sess:
        sess.admit(mu.to(DEV), [p.to(DEV) for p in prompts], steps, 0.0, noise=noise)
        assert sess.step(1) == [0, 1]
        before = sess.state
        assert before[2][0] == sess.LIVE and before[3][0] == sess.FREE
        assert _raw(cfm, [0, 2], [0, 50], ld, out) != 0                  # live
        assert _raw(cfm, [0, 3], [0, 50], ld, out) != 0                  # free
        assert _raw(cfm, [0, 4], [0, 50], ld, out) != 0 and _raw(cfm, [-1], [0], ld, out) != 0      # no such slot
        assert _raw(cfm, [0, 1, 0], [0, 40, 80], 200, out) != 0          # repeated
        assert _raw(cfm, [0], [0], ld, out, n=0) != 0 and _raw(cfm, [0] * 5, [0] * 5, ld, out, n=5) != 0
        for null in ("slots", "col0", "out"):
            assert _raw(cfm, [0], [0], ld, out, null=null) != 0
        assert _raw(cfm, [0, 1], [0, -1], ld, out) != 0                  # col0 < 0
        assert _raw(cfm, [0, 1], [0, ld - T + 1], ld, out) != 0          # slot 1: 40 frames from column 61 end at 101 > 100
        with pytest.raises(RuntimeError, match="fetch_mel"):
            sess.fetch_mel([0, 2], [0, 50], out, spec_min, spec_max)
        assert sess.state == before
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())
        assert _raw(cfm, [0, 1], [0, ld - T], ld, out) == 0              # the same call one column to the left fits exactly
        assert torch.equal(out[:, :T - 4], want[0]) and torch.equal(out[:, ld - T:], want[1])
        assert bool((out[:, T - 4:ld - T] == SENTINEL).all())
        assert [st[0] for st in sess.state] == [sess.FREE, sess.FREE, sess.LIVE, sess.FREE]


def test_full_size_geometry(cfm):
    """mel = 100, T = 934, the production chunk: Tp = 468 (the v3 prompt), 0 and 933, one Euler step of the small DiT each"""
    _check(cfm, 934, [468, 0, 933], [1, 1, 1], "mel934", gap=5)
