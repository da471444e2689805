"""CPU: which shapes gsv_op_conv_pair / gsv_op_conv_pair_seg accept at 64 channels (conv_pair64.hip), checked before anything
touches a device."""
import pytest


def _built_lib():
    from gsv import build, _lib
    build.build(verbose=False)
    return _lib


@pytest.mark.parametrize("dil", [1, 6])
def test_conv_pair_accepts_64_channels_for_exactly_the_instantiated_tap_counts(dil):
    """With null operands an accepted shape stops at launch_conv_pair's operand check, a refused one at the op's shape check.
    At C = 64 the accepted tap counts are exactly the instantiated kernels (3, 5, 7, 9, 11) within the span limit
    ((taps - 1) / 2 * dil <= 25): any other count would read tap slabs past the weights.  The masked op has no 64-channel
    kernel: gsv_op_conv_pair_seg stops at its shape check for every tap count."""
    import ctypes as C
    _lib = _built_lib()
    l = _lib.lib()
    accepted = []
    for taps in range(-13, 16):
        l.gsv_debug_last_conv_route(1)
        rc = l.gsv_op_conv_pair(None, None, None, None, None, None, 1024, 64, taps, dil, 1.0, 0, None)
        msg = l.gsv_last_error().decode()
        assert rc != 0 and l.gsv_debug_last_conv_route(1) == 0
        if "null operand" in msg:
            accepted.append(taps)
        else:
            assert "op_conv_pair: C must be" in msg, msg
        seg = (C.c_int32 * 1024)()
        rc = l.gsv_op_conv_pair_seg(None, None, None, None, None, None, 1024, 64, taps, dil, 1.0, 0, seg, None)
        msg = l.gsv_last_error().decode()
        assert rc != 0 and "op_conv_pair_seg: C must be" in msg, msg
    assert accepted == [k for k in (3, 5, 7, 9, 11) if (k - 1) // 2 * dil <= 25]
    rc = l.gsv_op_conv_pair(None, None, None, None, None, None, 1024, 48, 7, 1, 1.0, 0, None)
    assert rc != 0 and "op_conv_pair: C must be" in l.gsv_last_error().decode()
