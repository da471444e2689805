"""CPU: gsv_op_gemm_panel refuses every descriptor that is not one of the prefill's three GEMM forms before its first HIP call.
Without a device any HIP call would answer GSV_ERR_HIP; the refusal must be GSV_ERR_ARG, and no route is recorded."""
import ctypes as C

import pytest

from _gemm_panel_cases import GSV_ERR_ARG, REFUSALS, refusal_desc


def _built_lib():
    from gsv import build, _lib
    build.build(verbose=False)
    return _lib


@pytest.mark.parametrize("name", list(REFUSALS))
def test_gemm_panel_refuses_before_any_hip_call(name):
    _lib = _built_lib()
    l = _lib.lib()
    # addresses that are never dereferenced: 16-byte aligned, non-null
    d, dtype, tile = refusal_desc(_lib, name, 2304, 512, 512, x=0x10000, w=0x20000, bias=0x30000, y=0x40000, res=0x50000, gate=0x60000)
    l.gsv_debug_last_conv_route(1)
    rc = l.gsv_op_gemm_panel(C.byref(d), dtype, tile, None)
    assert rc == GSV_ERR_ARG, (name, rc, l.gsv_last_error().decode())
    assert "op_gemm_panel" in l.gsv_last_error().decode()
    assert l.gsv_debug_last_conv_route(1) == 0


def test_gemm_panel_refuses_a_null_descriptor():
    _lib = _built_lib()
    assert _lib.lib().gsv_op_gemm_panel(None, 1, 0, None) == GSV_ERR_ARG


def test_set_prefill_gemm_rejects_a_null_handle_and_is_exported():
    _lib = _built_lib()
    assert _lib.lib().gsv_t2s_set_prefill_gemm(None, 1) == GSV_ERR_ARG
