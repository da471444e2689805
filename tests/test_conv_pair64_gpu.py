"""GPU: the fused ResBlock pair at 64 channels (conv_pair64.hip) against the two launches it replaces, per element through
gsv_op_conv_pair / gsv_op_conv1d, and through an fp16 SynthesizerTrn.decode whose 64-channel stage is just above the
generator's threshold (T >= 16 384), with and without GSV_NO_CONV_PAIR64 in fresh child processes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CH = 64


def _conv(x_ct, w, bias, dil=1, res=None, scale=1.0, accumulate=None):
    """x_ct [C, T] fp32 cpu, w [C, C, k] -> y [C, T] through gsv_op_conv1d in fp16 with lrelu(0.1) on the input; returns the route too"""
    from gsv import _lib
    Cout, Cin, k = w.shape
    T = x_ct.shape[1]
    pad = (k * dil - dil) // 2
    x = x_ct.t().contiguous().to(DEV, torch.float16)
    wp = w.permute(0, 2, 1).reshape(Cout, k * Cin).contiguous().to(DEV, torch.float16)
    y = torch.zeros(T, Cout, device=DEV, dtype=torch.float16) if accumulate is None else accumulate.t().contiguous().to(DEV, torch.float16)
    b = bias.to(DEV, torch.float32).contiguous()
    r = res.t().contiguous().to(DEV, torch.float16) if res is not None else None
    d = _lib.ConvDesc(x.data_ptr(), wp.data_ptr(), b.data_ptr(), y.data_ptr(), r.data_ptr() if r is not None else None, T, T, Cin, Cout,
                      k, 1, dil, pad, 3, 0.1, 0, scale, 1 if accumulate is not None else 0, 0, 0, 0)
    _lib.check(_lib.lib().gsv_op_conv1d(C.byref(d), _lib.dtype_code(torch.float16), None))
    torch.cuda.synchronize()
    return y.float().cpu().t()


def _route():
    from gsv import _lib
    code = int(_lib.lib().gsv_debug_last_conv_route(1)) & 0xFFFFFFFFFFFFFFFF
    fam, c, taps, flags = code & 255, (code >> 16) & 255, (code >> 24) & 255, (code >> 56) & 255
    return f"conv_pair_f16<C{c},TAPS{taps},ACC{(flags >> 1) & 1}>" if fam == 8 else f"family {fam}"


def _case(k, dil, T, accum):
    torch.manual_seed(CH * 100 + k * 10 + dil)
    x = torch.randn(CH, T)
    w1, w2 = torch.randn(CH, CH, k) / (CH * k) ** 0.5, torch.randn(CH, CH, k) / (CH * k) ** 0.5
    b1, b2 = torch.randn(CH) * 0.1, torch.randn(CH) * 0.1
    y0 = torch.randn(CH, T) if accum else None
    return x, w1, b1, w2, b2, y0, (1.0 / 3.0 if accum else 1.0)


def _device_operands(x, w1, b1, w2, b2, k):
    pk = lambda w: w.permute(0, 2, 1).reshape(CH, k * CH).contiguous().to(DEV, torch.float16)
    return x.t().contiguous().to(DEV, torch.float16), pk(w1), b1.to(DEV), pk(w2), b2.to(DEV)


@pytest.mark.parametrize("k,dil,T,accum", [(11, 5, 2111, True), (3, 1, 256, False), (7, 3, 1025, False), (11, 1, 4500, True),
                                           (3, 5, 40000, False), (9, 2, 700, True), (5, 5, 3000, False)])
def test_pair64_matches_two_launches(k, dil, T, accum):
    """gsv_op_conv_pair at C = 64 vs convs1 then convs2 (+ x, * scale, optional accumulate) through gsv_op_conv1d: bit-identical
    fp16 without accumulate; with accumulate (scale 1/3) the allowance of test_conv_pair_matches_two_launches, which is the
    compiler's contraction of `* scale + y` and not this kernel's (|d| <= 1e-3 * (1 + |two|), fewer than 1e-3 of the elements
    differ).  Against the torch fp32 ResBlock pair <= 2e-2.  The cases: ragged last tile with the largest halo, one tile, one
    row past a tile edge (256-step tiles at 7 taps), 128-step tiles at 9 / 11 taps, the persistent loop, and the two tap
    counts the generator does not use."""
    from gsv import _lib
    _lib.init(0)
    x, w1, b1, w2, b2, y0, scale = _case(k, dil, T, accum)
    xh = x.half().float()
    t = _conv(xh, w1, b1, dil=dil)
    two = _conv(t, w2, b2, dil=1, res=xh, scale=scale, accumulate=y0.half().float() if accum else None)
    xd, w1d, b1d, w2d, b2d = _device_operands(x, w1, b1, w2, b2, k)
    yd = y0.t().contiguous().to(DEV, torch.float16) if accum else torch.zeros(T, CH, device=DEV, dtype=torch.float16)
    _lib.lib().gsv_debug_last_conv_route(1)
    _lib.check(_lib.lib().gsv_op_conv_pair(xd.data_ptr(), w1d.data_ptr(), b1d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), yd.data_ptr(),
                                           T, CH, k, dil, scale, 1 if accum else 0, None), "gsv_op_conv_pair")
    torch.cuda.synchronize()
    assert _route() == f"conv_pair_f16<C64,TAPS{k},ACC{int(accum)}>"
    fused = yd.float().cpu().t()
    d = (fused - two).abs()
    print(f"k {k} dil {dil} T {T} acc {accum}: max |fused - two| {d.max():.3e}, differing {(d > 0).float().mean():.3e}")
    if accum:
        assert (d <= 1e-3 * (1 + two.abs())).all() and (d > 0).float().mean() < 1e-3
    else:
        assert torch.equal(fused, two), f"max diff {d.max()}"
    ref = F.conv1d(F.leaky_relu(xh, 0.1).unsqueeze(0), w1.half().float(), b1, dilation=dil, padding=(k - 1) // 2 * dil)
    ref = F.conv1d(F.leaky_relu(ref, 0.1), w2.half().float(), b2, padding=(k - 1) // 2)[0]
    ref = (ref + xh) * scale + (y0.half().float() if accum else 0)
    assert (fused - ref).abs().max() <= 2e-2


def test_pair64_in_place_is_refused():
    """y == x is REFUSED at C = 64 (rc != 0, nothing launched, x untouched): the kernel reads rows of x that belong to other
    workgroups' tiles as halo, so writing y over x would race.  The generator never asks for it: it swaps buffers
    (run_generator_stages, `pa.y == xr -> xt`)."""
    from gsv import _lib
    _lib.init(0)
    k, dil, T = 7, 3, 1025
    x, w1, b1, w2, b2, _, _ = _case(k, dil, T, False)
    xd, w1d, b1d, w2d, b2d = _device_operands(x, w1, b1, w2, b2, k)
    before = xd.clone()
    _lib.lib().gsv_debug_last_conv_route(1)
    rc = _lib.lib().gsv_op_conv_pair(xd.data_ptr(), w1d.data_ptr(), b1d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(), xd.data_ptr(),
                                     T, CH, k, dil, 1.0, 0, None)
    torch.cuda.synchronize()
    assert rc != 0 and "in place" in _lib.lib().gsv_last_error().decode()
    assert _lib.lib().gsv_debug_last_conv_route(1) == 0 and torch.equal(xd, before)


# ---- engine level: an fp16 decode whose 64-channel stage has 160 * 104 = 16 640 rows, just above the threshold (16 384)
N_CODES = 52          # 104 frames


def _decode_wave():
    from gsv import synthetic as S
    from gsv.module.models import SynthesizerTrn
    cfg = S.VITS_V2_CONFIG
    d, mk = cfg["data"], dict(cfg["model"])
    version = mk.pop("version", "v2")
    m = SynthesizerTrn(d["filter_length"] // 2 + 1, cfg["train"]["segment_size"] // d["hop_length"], n_speakers=d["n_speakers"],
                       version=version, device=DEV, dtype=torch.float16, n_symbols=cfg["n_symbols"], **mk)
    m.load_state_dict(S.make_vits_state_dict(cfg, seed=3))
    codes = torch.from_numpy(S.hash_ints("pair64_codes", N_CODES, 1024, 5)).view(1, 1, -1).to(DEV)
    text = torch.from_numpy(S.hash_ints("pair64_text", 23, cfg["n_symbols"], 5)).view(1, -1).to(DEV)
    refer = torch.from_numpy(S.hash_uniform("pair64_refer", 1025 * 21, 11).reshape(1, 1025, 21).copy()).to(DEV)
    return m.decode(codes, text, refer, seed=4321).float().cpu().numpy().reshape(-1)


if __name__ == "__main__":
    # child process of test_decode_with_and_without_the_pair: the decode under the switches of this process's environment
    np.save(sys.argv[1], _decode_wave())
    sys.exit(0)


def _child(tmp_path, name, **switches):
    path = str(tmp_path / f"{name}.npy")
    env = dict(os.environ, **switches)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "gpt-sovits_amd"), os.path.join(ROOT, "tests"), env.get("PYTHONPATH", "")])
    child = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), path], env=env, cwd=ROOT,
                           capture_output=True, text=True)
    assert child.returncode == 0, f"child {name} exited {child.returncode}:\n{child.stdout[-2000:]}\n{child.stderr[-2000:]}"
    return np.load(path).astype(np.float64)


def test_decode_with_and_without_the_pair(tmp_path):
    """The same fp16 decode in three fresh processes: default, GSV_NO_CONV_PAIR64=1 (the 64-channel stage as two conv_narrow
    launches per pair) and GSV_NO_CONV_PAIR=1 (no fused pair at all).  The 64-channel pair may change the waveform by no more
    than the 16 / 32-channel pairs already do: zero, or the accumulate pairs' one-ulp cases carried through."""
    assert 160 * 2 * N_CODES >= 16384 > 160 * 2 * (N_CODES - 1)
    default = _child(tmp_path, "default")
    no64 = _child(tmp_path, "no64", GSV_NO_CONV_PAIR64="1")
    none = _child(tmp_path, "none", GSV_NO_CONV_PAIR="1")
    assert default.shape == no64.shape == none.shape and np.isfinite(default).all() and np.abs(default).max() > 0
    d64, dall = float(np.abs(default - no64).max()), float(np.abs(default - none).max())
    print(f"max |default - GSV_NO_CONV_PAIR64| {d64:.3e}; max |default - GSV_NO_CONV_PAIR| {dall:.3e}")
    assert d64 <= dall
