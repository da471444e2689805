"""GPU: the segmented SoVITS decode through the masked fused ResBlock pairs (conv_pair.hip SEG) of its 32- and 16-channel
generator stages: the route is taken, it agrees with the unfused path (GSV_NO_SEG_PAIR=1, in a child process), nothing
leaks across a segment boundary and the gap rows stay 0."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gsv import synthetic as S
from test_vits_segments_gpu import CODE_LENS, PHONE_LENS, _engine, _seg_inputs, _six, _voice

pytestmark = pytest.mark.gpu
SEG_FLAG = 16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair_route():
    from gsv import _lib
    code = int(_lib.lib().gsv_debug_last_pair_route(1)) & 0xFFFFFFFFFFFFFFFF
    return code & 255, (code >> 16) & 255, (code >> 24) & 255, (code >> 56) & 255


def _segments(cname):
    """small: the six segments of test_vits_segments_gpu (859 frames: 6872 and 13744 rows in the 32- and 16-channel stages);
    v2: 8 segments x 100 codes, 8 voices"""
    if cname == "small":
        return _six(None)
    segs = []
    for i in range(8):
        codes, text = _seg_inputs(100, 20 + (i * 7) % 31, f"pair{i}")
        segs.append((codes, text, _voice(200 + i, tr=20 + i), 9000 + i))
    return segs


def _decode(cname):
    m, cfg, _ = _engine(cname, torch.float16)
    segs = _segments(cname)
    out = m.decode_segments([s[0] for s in segs], [s[1] for s in segs], [s[2] for s in segs], [s[3] for s in segs])
    return m, cfg, segs, out


@pytest.mark.parametrize("cname", ["small", "v2"])
def test_segmented_decode_takes_the_masked_pair(cname):
    from gsv import _lib
    _lib.lib().gsv_debug_last_pair_route(1)
    m, cfg, segs, out = _decode(cname)
    fam, c, taps, flags = _pair_route()
    last_ch = cfg["model"]["upsample_initial_channel"] >> len(cfg["model"]["upsample_rates"])
    assert fam == 8 and flags & SEG_FLAG, (fam, c, taps, flags)
    assert c == last_ch and taps == cfg["model"]["resblock_kernel_sizes"][-1]
    assert all(torch.isfinite(o).all() for o in out)
    # one segment keeps the plain decode, and with it the unmasked pair
    m.decode_segments([segs[3][0]], [segs[3][1]], [segs[3][2]], [segs[3][3]])
    fam, _, _, flags = _pair_route()
    assert fam == 8 and not flags & SEG_FLAG


if __name__ == "__main__":
    # child process of test_fused_against_unfused: the same segments with the switch of this process's environment
    cname, path = sys.argv[1], sys.argv[2]
    from gsv import _lib
    _lib.lib().gsv_debug_last_pair_route(1)
    _, _, _, out = _decode(cname)
    fam, _, _, flags = _pair_route()
    np.savez(path, route=np.array([fam, flags]), **{f"w{i}": o.float().cpu().numpy().reshape(-1) for i, o in enumerate(out)})
    sys.exit(0)


@pytest.mark.parametrize("cname", ["small", "v2"])
def test_fused_against_unfused(cname, tmp_path):
    """The op-level bar (1e-3 * (1 + |ref|), accumulate pairs only) does not carry through conv_post and tanh unchanged, so
    the waveforms are held to the fp16 bar the project holds against fp32 (2e-2 max-abs, 3 % relative rms;
    test_production_shape_fp16).  Measured on MI355X: see DESIGN.md section 4e."""
    _, _, segs, fused = _decode(cname)
    path = str(tmp_path / "unfused.npz")
    env = dict(os.environ, GSV_NO_SEG_PAIR="1")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "gpt-sovits_amd"), os.path.join(ROOT, "tests"),
                                         env.get("PYTHONPATH", "")])
    child = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), cname, path], env=env,
                           cwd=ROOT, capture_output=True, text=True)
    assert child.returncode == 0, f"unfused child exited {child.returncode}:\n{child.stdout[-2000:]}\n{child.stderr[-2000:]}"
    ref = np.load(path)
    assert int(ref["route"][0]) == 0, "GSV_NO_SEG_PAIR=1 still launched a fused pair"
    worst, worst_rel = 0.0, 0.0
    for i, o in enumerate(fused):
        a, b = o.float().cpu().numpy().reshape(-1).astype(np.float64), ref[f"w{i}"].astype(np.float64)
        assert a.shape == b.shape
        worst = max(worst, float(np.abs(a - b).max()))
        worst_rel = max(worst_rel, float(np.sqrt(np.mean((a - b) ** 2)) / max(np.sqrt(np.mean(b ** 2)), 1e-12)))
    print(f"{cname}: fused vs unfused segmented decode, max-abs {worst:.3e}, relative rms {worst_rel:.3e}")
    assert worst <= 2e-2 and worst_rel <= 3e-2


def test_no_leakage_through_the_fused_pairs():
    from gsv import _lib
    m, _, _ = _engine("small", torch.float16)
    outs = []
    for swap in (False, True):
        segs = _six(m, swap2=swap)
        _lib.lib().gsv_debug_last_pair_route(1)
        outs.append(m.decode_segments([s[0] for s in segs], [s[1] for s in segs], [s[2] for s in segs], [s[3] for s in segs]))
        assert _pair_route()[3] & SEG_FLAG
    for i in range(6):
        if i != 2:
            assert torch.equal(outs[0][i], outs[1][i]), f"segment {i} changed when segment 2 changed"
    assert not torch.equal(outs[0][2], outs[1][2])


def test_gap_rows_of_the_stage_outputs_are_zero():
    from gsv import _lib
    m, cfg, segs, _ = _decode("small")
    assert _pair_route()[3] & SEG_FLAG
    mc = cfg["model"]
    vc = _lib.VitsConfig()
    vc.kernel_size = mc["kernel_size"]
    vc.n_ups = len(mc["upsample_rates"])
    for i, (u, k) in enumerate(zip(mc["upsample_rates"], mc["upsample_kernel_sizes"])):
        vc.up_rates[i], vc.up_kernels[i] = u, k
    vc.n_resblocks = len(mc["resblock_kernel_sizes"])
    for j, (k, ds) in enumerate(zip(mc["resblock_kernel_sizes"], mc["resblock_dilation_sizes"])):
        vc.rb_kernels[j] = k
        for c, d in enumerate(ds):
            vc.rb_dilations[j][c] = d
    n = len(CODE_LENS)
    cl, pl = (C.c_int * n)(*CODE_LENS), (C.c_int * n)(*PHONE_LENS)
    level = vc.n_ups - 1                       # the last stage's input = the 32-channel stage's output, all of it fused pairs
    rows = C.c_int64(0)
    _lib.check(_lib.lib().gsv_vits_segment_map(C.byref(vc), n, cl, pl, level, None, 0, C.byref(rows)))
    buf = (C.c_int32 * rows.value)()
    _lib.check(_lib.lib().gsv_vits_segment_map(C.byref(vc), n, cl, pl, level, buf, rows.value, C.byref(rows)))
    sl = np.frombuffer(buf, dtype=np.int32)
    ch = 2 * (mc["upsample_initial_channel"] >> vc.n_ups)
    assert ch == 32
    g = m.debug_tensor("gen_last_in", ch * len(sl)).cpu().numpy().reshape(ch, len(sl))
    assert (sl < 0).any() and np.all(g[:, sl < 0] == 0) and np.abs(g[:, sl >= 0]).max() > 0
