"""CPU: the packed layout of the speaker-embedding pass (gsv.eres2net.ERes2NetV2.plan_segments) and the
declaration of its two kernels.  Frame counts 9, 16, 23, 101, 8, 1: a multiple of 8, odd counts at every stride level, a
single frame; with one large pass and with max_frames = 64 (several passes, one audio larger than a pass)."""
import os
import re

import pytest

from conftest import ROOT

COUNTS = [9, 16, 23, 101, 8, 1]


def _plan(max_frames):
    from gsv.eres2net.ERes2NetV2 import plan_segments
    return plan_segments(COUNTS, max_frames)


@pytest.mark.parametrize("max_frames", [1 << 20, 64])
def test_slots_levels_and_gaps(max_frames):
    plan = _plan(max_frames)
    assert [s for ps in plan for s in ps["audios"]] == list(range(len(COUNTS)))                    # the order is kept
    for ps in plan:
        assert ps["m"] == [COUNTS[s] for s in ps["audios"]]
        slots = [8 * (-(-m // 8) + 1) for m in ps["m"]]
        assert ps["frames"] == sum(slots) and ps["frames"] % 8 == 0
        assert ps["slot_start"] == [sum(slots[:i]) for i in range(len(slots))]
        assert all(o % 8 == 0 for o in ps["slot_start"])
        assert len(ps["levels"]) == 4
        for k, lv in enumerate(ps["levels"]):
            assert lv["rows"] == ps["frames"] >> k
            assert lv["seg_start"] == [o >> k for o in ps["slot_start"]]
            assert lv["seg_len"] == [-(-m // (1 << k)) for m in ps["m"]]
            ends = [a + n for a, n in zip(lv["seg_start"], lv["seg_len"])]
            for i, e in enumerate(ends):                                                           # at least one gap row behind each
                nxt = lv["seg_start"][i + 1] if i + 1 < len(ends) else lv["rows"]
                assert e + 1 <= nxt
            inside = {r for a, n in zip(lv["seg_start"], lv["seg_len"]) for r in range(a, a + n)}
            assert lv["gap_rows"] == [r for r in range(lv["rows"]) if r not in inside]
            assert all(e in lv["gap_rows"] for e in ends)


def test_passes_respect_max_frames():
    one = _plan(1 << 20)
    assert len(one) == 1 and one[0]["frames"] == 24 + 24 + 32 + 112 + 16 + 16
    plan = _plan(64)
    assert [ps["audios"] for ps in plan] == [[0, 1], [2], [3], [4, 5]]
    for ps in plan:
        assert ps["frames"] <= 64 or len(ps["audios"]) == 1
    assert plan[2]["frames"] == 112                                                                # the lone oversized audio


def test_hard_cap_on_the_largest_map():
    from gsv.eres2net.ERes2NetV2 import plan_segments
    m = 40000                                               # 40008 slot frames x 82 x 256 = 8.4e8 elements: two fit below 2^31, three do not
    plan = plan_segments([m] * 5, 1 << 30)
    assert [len(ps["audios"]) for ps in plan] == [2, 2, 1]
    assert all(ps["frames"] * 82 * 256 < 1 << 31 for ps in plan)
    with pytest.raises(ValueError):
        plan_segments([110000], 1 << 30)                    # one audio alone is past the cap


@pytest.mark.parametrize("counts", [[9, 0, 3], [0], [5, -1]])
def test_audio_without_a_frame_is_refused(counts):
    from gsv.eres2net.ERes2NetV2 import plan_segments
    with pytest.raises(ValueError):
        plan_segments(counts, 1 << 20)


def test_new_entries_are_declared_and_exported():
    from gsv import _lib
    src = open(os.path.join(ROOT, "include", "gsv.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gsv_op_zero_rows", "gsv_op_time_mean_seg"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in include/gsv.h"
        assert name in _lib.EXPORTS
    assert re.search(r"int gsv_abi_version\(void\) \{ return 1; \}", open(os.path.join(ROOT, "gpt-sovits_amd", "csrc", "ops.hip")).read())
    from gsv import build
    build.build(verbose=False)
    l = _lib.lib()
    assert hasattr(l, "gsv_op_zero_rows") and hasattr(l, "gsv_op_time_mean_seg") and l.gsv_abi_version() == 1
