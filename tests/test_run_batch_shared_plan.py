"""CPU: the waveform launch plan of TTS.run_batch(shared_sovits=True) -- which folds share a segmented SoVITS pass and
where a pass is cut -- for hand-made plans.  Frame counts are checked against the library's own layout
(gsv_vits_segment_gap / gsv_vits_segment_map, host-only)."""
import ctypes as C
import inspect
from types import SimpleNamespace

from gsv import build, synthetic as S
from gsv.TTS_infer_pack.TTS import TTS


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


MODEL = S.VITS_V2_CONFIG["model"]


def _gap():
    lib = _lib()
    return lib.lib().gsv_vits_segment_gap(C.byref(_vc(lib, MODEL)))


def _frames(code_lens):
    """rows of the frame-level segment map of these folds in one pass"""
    lib = _lib()
    n = len(code_lens)
    rows = C.c_int64(0)
    assert lib.lib().gsv_vits_segment_map(C.byref(_vc(lib, MODEL)), n, (C.c_int * n)(*code_lens), (C.c_int * n)(*([1] * n)), 0,
                                          None, 0, C.byref(rows)) == 0
    return rows.value


def _stub(max_frames, use_vocoder=False):
    return SimpleNamespace(configs=SimpleNamespace(use_vocoder=use_vocoder), sovits_max_frames=max_frames,
                           vits_model=SimpleNamespace(segment_gap=_gap), _voice_key=TTS._voice_key)


def _voice():
    return {"refer_spec": [object()], "sv_emb": None}


def _plan(voice, folds, speed=1.0):
    return dict(voice=voice, folds=list(folds), opts=TTS._request_options({"speed_factor": speed}))


def _check(launches, plans, max_frames, shareable):
    flat = [e for L in launches for e in L]
    assert sorted(flat) == sorted(shareable) and len(set(flat)) == len(flat)
    for L in launches:
        assert L == sorted(L) and len(L) >= 1
        assert len({TTS._voice_key(plans[r]["voice"]) for r, _ in L}) <= 128
        assert len(L) == 1 or _frames([plans[r]["folds"][bi] for r, bi in L]) <= max_frames
    assert [L[0] for L in launches] == sorted(L[0] for L in launches)


def test_keyword_and_class_attribute():
    assert inspect.signature(TTS.run_batch).parameters["shared_sovits"].default is False
    assert TTS.sovits_max_frames == 25600


def test_what_is_shared_and_where_a_pass_is_cut():
    va, vb = _voice(), _voice()
    plans = [_plan(va, [100, 40]),           # two to_batch batches: two folds
             _plan(vb, [60], speed=1.25),    # speed != 1: not shared
             _plan(vb, [0, 30]),             # an empty fold is left to run()'s path
             _plan(va, [120]),
             _plan(_voice(), [])]            # no text
    shareable = [(0, 0), (0, 1), (2, 1), (3, 0)]
    big = 10 ** 6
    launches = TTS.plan_sovits(_stub(big), plans)
    assert launches == [shareable]
    _check(launches, plans, big, shareable)
    # a cap that the four folds exceed together: 2 * (100 + 40 + 30 + 120) + 3 gaps
    total = _frames([100, 40, 30, 120])
    assert total == 2 * 290 + 3 * _gap()
    launches = TTS.plan_sovits(_stub(total), plans)
    assert launches == [shareable]
    launches = TTS.plan_sovits(_stub(total - 1), plans)
    assert launches == [[(0, 0), (0, 1), (2, 1)], [(3, 0)]]
    _check(launches, plans, total - 1, shareable)
    # a single fold above the cap gets a pass of its own
    launches = TTS.plan_sovits(_stub(150), plans)
    assert launches == [[(0, 0)], [(0, 1), (2, 1)], [(3, 0)]]
    _check(launches, plans, 150, shareable)


def test_v3_shares_nothing():
    plans = [_plan(_voice(), [50]), _plan(_voice(), [70])]
    assert TTS.plan_sovits(_stub(10 ** 6, use_vocoder=True), plans) == []


def test_voice_slots_bound_a_pass():
    voices = [_voice() for _ in range(130)]
    plans = [_plan(v, [10]) for v in voices]
    launches = TTS.plan_sovits(_stub(10 ** 6), plans)
    assert [len(L) for L in launches] == [128, 2]
    _check(launches, plans, 10 ** 6, [(r, 0) for r in range(130)])
    # two requests with one voice count once: 129 requests over 128 voices fit one pass
    plans = [_plan(v, [10]) for v in voices[:128]] + [_plan(voices[5], [10])]
    launches = TTS.plan_sovits(_stub(10 ** 6), plans)
    assert [len(L) for L in launches] == [129]
    # voices taken from one prompt cache are one voice (the same stored spectrogram list), whatever dict carries them
    a = _voice()
    b = dict(a)
    assert TTS._voice_key(a) == TTS._voice_key(b) != TTS._voice_key(_voice())
