"""CPU: the waveform launch plan of TTS.run_batch(shared_sovits=True, shared_speed=True) -- which speed-1 folds and which
sentences of requests at another speed share a segmented SoVITS pass, and where a pass is cut -- for hand-made plans.
A row costs the larger of its frame counts before and after the speed interpolation; both are checked against the
library's own layouts (gsv_vits_segment_map / gsv_vits_segment_map_speed, host-only)."""
import ctypes as C
import inspect
from types import SimpleNamespace

from gsv import build, synthetic as S
from gsv.TTS_infer_pack.TTS import TTS

MODEL = S.VITS_V2_CONFIG["model"]


def _lib():
    from gsv import _lib
    build.build(verbose=False)
    return _lib


def _vc(lib, model):
    vc = lib.VitsConfig()
    vc.kernel_size = model["kernel_size"]
    vc.n_ups = len(model["upsample_rates"])
    for i, (u, k) in enumerate(zip(model["upsample_rates"], model["upsample_kernel_sizes"])):
        vc.up_rates[i], vc.up_kernels[i] = u, k
    vc.n_resblocks = len(model["resblock_kernel_sizes"])
    for j, (k, ds) in enumerate(zip(model["resblock_kernel_sizes"], model["resblock_dilation_sizes"])):
        vc.rb_kernels[j] = k
        for c, d in enumerate(ds):
            vc.rb_dilations[j][c] = d
    return vc


def _gap():
    lib = _lib()
    return lib.lib().gsv_vits_segment_gap(C.byref(_vc(lib, MODEL)))


def _frames(code_lens, speeds):
    """frame rows, gaps included, of these segments in one pass: (pre layout, post layout)"""
    lib = _lib()
    n = len(code_lens)
    cl, pl, rows = (C.c_int * n)(*code_lens), (C.c_int * n)(*([1] * n)), C.c_int64(0)
    assert lib.lib().gsv_vits_segment_map(C.byref(_vc(lib, MODEL)), n, cl, pl, 0, None, 0, C.byref(rows)) == 0
    pre = rows.value
    assert lib.lib().gsv_vits_segment_map_speed(C.byref(_vc(lib, MODEL)), n, cl, pl, (C.c_double * n)(*speeds), 0, None, 0,
                                                C.byref(rows)) == 0
    return pre, rows.value


def _stub(max_frames, use_vocoder=False):
    return SimpleNamespace(configs=SimpleNamespace(use_vocoder=use_vocoder), sovits_max_frames=max_frames,
                           vits_model=SimpleNamespace(segment_gap=_gap), _voice_key=TTS._voice_key)


def _voice():
    return {"refer_spec": [object()], "sv_emb": None}


def _plan(voice, sentences, speed=1.0):
    """sentences[bi][k] = kept tokens of sentence k of to_batch batch bi"""
    return dict(voice=voice, sentences=[list(s) for s in sentences], folds=[sum(s) for s in sentences],
                opts=TTS._request_options({"speed_factor": speed}))


def _tokens(plans, row):
    r, bi, k = row
    return plans[r]["folds"][bi] if k < 0 else plans[r]["sentences"][bi][k]


def _check(launches, plans, max_frames, shareable):
    flat = [e for L in launches for e in L]
    assert flat == sorted(shareable) and len(set(flat)) == len(flat)            # (r, bi, k) order, across launches too
    for L in launches:
        assert len(L) >= 1
        assert len({TTS._voice_key(plans[r]["voice"]) for r, _, _ in L}) <= 128
        for r, _, k in L:
            assert (k == -1) == (plans[r]["opts"]["speed_factor"] == 1.0)
        pre, post = _frames([_tokens(plans, e) for e in L], [plans[e[0]]["opts"]["speed_factor"] for e in L])
        assert len(L) == 1 or max(pre, post) <= max_frames


def test_keyword_defaults():
    p = inspect.signature(TTS.run_batch).parameters
    assert p["shared_speed"].default is False and p["shared_sovits"].default is False and p["shared_cfm"].default is False


def _mix():
    va, vb = _voice(), _voice()
    plans = [_plan(va, [[60, 40], [40]]),                  # speed 1: two folds, shared whole
             _plan(vb, [[30, 0, 30]], speed=1.25),         # faster: sentences 0 and 2; the empty one is left out
             _plan(vb, [[0], [30]]),                       # an empty fold is left to run()'s path
             _plan(va, [[50], [0, 0], [20, 25]], speed=0.8),   # slower: three sentences over two batches; batch 1 is empty
             _plan(va, [[120]]),
             _plan(_voice(), [])]                          # no text
    shareable = [(0, 0, -1), (0, 1, -1), (1, 0, 0), (1, 0, 2), (2, 1, -1), (3, 0, 0), (3, 2, 0), (3, 2, 1), (4, 0, -1)]
    return plans, shareable


def test_what_is_shared():
    plans, shareable = _mix()
    big = 10 ** 6
    launches = TTS.plan_sovits_rows(_stub(big), plans)
    assert launches == [shareable]
    _check(launches, plans, big, shareable)
    # plan_sovits is what it was: the speed requests are not in it
    assert TTS.plan_sovits(_stub(big), plans) == [[(0, 0), (0, 1), (2, 1), (4, 0)]]


def test_v3_shares_nothing():
    plans = [_plan(_voice(), [[50]]), _plan(_voice(), [[70]], speed=1.25)]
    assert TTS.plan_sovits_rows(_stub(10 ** 6, use_vocoder=True), plans) == []


def test_a_pass_is_cut_at_the_larger_frame_count():
    plans, shareable = _mix()
    G = _gap()
    # per row max(2T, F_s): 1.25 -> 2T (F_s = int(60 / 1.25) + 1 = 49); 0.8 -> F_s (126, 51, 63)
    cost = [200, 80, 60, 60, 60, 126, 51, 63, 240]
    assert [max(2 * t, 2 * t if s == 1.0 else int(2 * t / s) + 1) for t, s in
            [(_tokens(plans, e), plans[e[0]]["opts"]["speed_factor"]) for e in shareable]] == cost
    total = sum(cost) + 8 * G
    assert TTS.plan_sovits_rows(_stub(total), plans) == [shareable]
    launches = TTS.plan_sovits_rows(_stub(total - 1), plans)
    assert launches == [shareable[:8], shareable[8:]]
    _check(launches, plans, total - 1, shareable)
    # the slow sentence (3, 0, 0) is 100 frames before the interpolation and 126 after: a cap between the two cuts before it
    head = sum(cost[:5]) + 4 * G
    assert TTS.plan_sovits_rows(_stub(head + G + 126), plans)[0] == shareable[:6]
    assert TTS.plan_sovits_rows(_stub(head + G + 125), plans)[0] == shareable[:5]
    # the fast sentence (1, 0, 0) is 60 frames before and 49 after: it is cut at 60
    head = sum(cost[:2]) + G
    assert TTS.plan_sovits_rows(_stub(head + G + 60), plans)[0] == shareable[:3]
    launches = TTS.plan_sovits_rows(_stub(head + G + 59), plans)
    assert launches[0] == shareable[:2]
    _check(launches, plans, head + G + 59, shareable)
    # a row above the cap gets a pass of its own
    launches = TTS.plan_sovits_rows(_stub(130), plans)
    assert [(4, 0, -1)] in launches and [(0, 0, -1)] in launches
    _check(launches, plans, 130, shareable)


def test_voice_slots_bound_a_pass():
    voices = [_voice() for _ in range(130)]
    plans = [_plan(v, [[10]], speed=1.0 if i % 2 else 1.5) for i, v in enumerate(voices)]
    launches = TTS.plan_sovits_rows(_stub(10 ** 6), plans)
    assert [len(L) for L in launches] == [128, 2]
    _check(launches, plans, 10 ** 6, [(r, 0, -1 if r % 2 else 0) for r in range(130)])
    # the sentences of one request are one voice
    plans = [_plan(v, [[10]]) for v in voices[:127]] + [_plan(voices[127], [[5, 5, 5]], speed=0.9)]
    assert [len(L) for L in TTS.plan_sovits_rows(_stub(10 ** 6), plans)] == [130]
