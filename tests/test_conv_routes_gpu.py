"""GPU: every kernel instantiation behind gsv_op_conv1d / gsv_op_conv_pair, each pinned by name and checked per element.

For every row of tests/_conv_routes.py (shape, flags, expected route, why):
  * the launch recorded the expected instantiation (gsv_debug_last_conv_route), so a moved dispatch threshold fails here
    instead of silently checking another kernel;
  * every output element is within the bar derived in tests/_convref.py from the fp64 mirror of the kernel's arithmetic;
  * rows after T_out and columns outside the [y_col0, y_col0 + Cout) slice of each ldy row still hold a NaN sentinel;
  * a second launch on the same inputs is bit-identical (persistent tile schedulers, split-K sums).
"""
import ctypes as C
import math
import zlib

import pytest
import torch

import _convref as R
from _conv_routes import CASES, PAIR_CASES, decode_route

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 3                                          # sentinel rows after T_out
SENT = {torch.float16: (torch.int16, 0x7E5A), torch.float32: (torch.int32, 0x7FC0DEAD)}   # quiet NaNs no kernel writes


def _gen(name):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(name.encode()))
    return g


def _sentinel(shape, dtype):
    it, v = SENT[dtype]
    return torch.full(shape, v, dtype=it, device=DEV).view(dtype)


def _route():
    from gsv import _lib
    return decode_route(_lib.lib().gsv_debug_last_conv_route(1))


def _bits(t):
    return t.view(SENT[t.dtype][0])


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_conv_route(case):
    from gsv import _lib
    _lib.init(0)
    dt = torch.float16 if case.dtype == "f16" else torch.float32
    g = _gen(case.name)
    Z, Cin, Cout, taps = case.Z, case.Cin, case.Cout, case.taps
    cr = Cout // case.ups if case.ups else Cout
    pad = case.pad if case.pad >= 0 else (taps - 1) * abs(case.dil) // 2
    if case.ups:
        T_out, T_virt = case.T * case.ups, case.T + taps - 1
    else:
        T_out = (case.T + 2 * pad - case.dil * (taps - 1) - 1) // case.stride + 1
        T_virt = T_out
    ydt = torch.float32 if case.out_f32 else dt
    rdt = {0: ydt, 1: torch.float32, 2: dt}[case.res_dtype]
    ldy = case.ldy or case.y_col0 + cr
    rows = T_out + GUARD
    bz = cr if Z > 1 else 0
    x = torch.randn(Z, case.T, Cin, generator=g).to(dt)
    w = (torch.randn(Z, Cout, taps, Cin, generator=g) / math.sqrt(taps * Cin)).to(dt)
    bias = torch.randn(max(Z * bz, cr), generator=g) * 0.5
    gate = torch.rand(max(Z * bz, cr), generator=g) + 0.5 if case.gate else None
    res = torch.randn(Z, T_out, cr, generator=g).to(rdt) if case.res else None
    y_prev = torch.randn(Z, T_out, cr, generator=g).to(ydt) if case.acc else None

    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    gd = gate.to(DEV) if gate is not None else None
    rd = res.to(DEV) if res is not None else None
    y0 = _sentinel((Z, rows, ldy), ydt)
    if y_prev is not None:
        y0[:, :T_out, case.y_col0:case.y_col0 + cr] = y_prev.to(DEV)
    d = _lib.ConvDesc(x=xd.data_ptr(), w=wd.data_ptr(), bias=bd.data_ptr(), y=0, res=rd.data_ptr() if rd is not None else None,
                      T_in=case.T, T_out=T_out, Cin=Cin, Cout=Cout, taps=taps, stride=case.stride, dil=case.dil, pad=pad,
                      pre_act=case.pre, pre_slope=case.slope, post_act=case.post, scale=case.scale, accumulate=int(case.acc),
                      out_f32=int(case.out_f32), ups_u=case.ups, ups_pad=case.ups_pad, Z=Z, xz=case.T * Cin,
                      wz=Cout * taps * Cin, yz=rows * ldy, ldx=Cin, ldw=taps * Cin, ldy=ldy,
                      gate=gd.data_ptr() if gd is not None else None, bz=bz, rz=T_out * cr, ldr=cr, res_dtype=case.res_dtype,
                      y_col0=case.y_col0, w_nt=int(case.w_nt), z_res=int(case.z_res))
    outs, routes = [], []
    for _ in range(2):
        y = y0.clone()
        d.y = y.data_ptr()
        _lib.lib().gsv_debug_last_conv_route(1)
        _lib.check(_lib.lib().gsv_op_conv1d(C.byref(d), _lib.dtype_code(dt), None), case.name)
        routes.append(_route())
        torch.cuda.synchronize()
        outs.append(y.cpu())
    assert routes[0] == routes[1] == case.route, f"{case.name}: launched {routes[0]}, expected {case.route} ({case.why})"
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), f"{case.name}: second launch differs"
    y = outs[0]
    inside = torch.zeros(Z, rows, ldy, dtype=torch.bool)
    inside[:, :T_out, case.y_col0:case.y_col0 + cr] = True
    assert torch.all(_bits(y)[~inside] == SENT[ydt][1]), f"{case.name}: stray writes outside the output slice"

    ref, bar = R.conv_mirror(x=x, w=w, bias=bias, gate=gate, res=res, y_prev=y_prev, dtype=dt, out_dtype=ydt, T_out=T_out,
                             T_virt=T_virt, stride=case.stride, dil=case.dil, pad=pad, pre=case.pre, slope=case.slope,
                             post=case.post, scale=case.scale, ups_u=case.ups, ups_pad=case.ups_pad, bz=bz)
    worst = R.check(y[:, :T_out, case.y_col0:case.y_col0 + cr], ref, bar, case.name)
    print(f"[route] {case.name} {routes[0]} worst err/bar {worst:.3f}")


@pytest.mark.parametrize("C_,taps,acc,T,dil", PAIR_CASES, ids=[f"c{c}_k{k}_a{a}" for c, k, a, _, _ in PAIR_CASES])
def test_conv_pair_route(C_, taps, acc, T, dil):
    """fused ResBlock pair vs the fp64 mirror of the pair (not only vs the two-launch path), every TAPS x C x ACCU"""
    from gsv import _lib
    _lib.init(0)
    g = _gen(f"pair{C_}_{taps}_{acc}")
    x = torch.randn(T, C_, generator=g).half()
    w1 = (torch.randn(C_, taps, C_, generator=g) / math.sqrt(taps * C_)).half()
    w2 = (torch.randn(C_, taps, C_, generator=g) / math.sqrt(taps * C_)).half()
    b1, b2 = torch.randn(C_, generator=g) * 0.1, torch.randn(C_, generator=g) * 0.1
    y_prev = torch.randn(T, C_, generator=g).half() if acc else None
    scale = 1.0 / 3.0 if acc else 1.0
    xd, w1d, w2d, b1d, b2d = x.to(DEV), w1.to(DEV), w2.to(DEV), b1.to(DEV), b2.to(DEV)
    y0 = _sentinel((T + GUARD, C_), torch.float16)
    if acc:
        y0[:T] = y_prev.to(DEV)
    outs, routes = [], []
    for _ in range(2):
        y = y0.clone()
        _lib.lib().gsv_debug_last_conv_route(1)
        _lib.check(_lib.lib().gsv_op_conv_pair(xd.data_ptr(), w1d.data_ptr(), b1d.data_ptr(), w2d.data_ptr(), b2d.data_ptr(),
                                               y.data_ptr(), T, C_, taps, dil, scale, int(acc), None), "gsv_op_conv_pair")
        routes.append(_route())
        torch.cuda.synchronize()
        outs.append(y.cpu())
    want = f"conv_pair_f16<C{C_},TAPS{taps},ACC{int(acc)}>"
    assert routes[0] == routes[1] == want, routes
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    assert torch.all(_bits(outs[0][T:]) == SENT[torch.float16][1]), "stray writes after T"
    ref, bar = R.pair_mirror(x=x, w1=w1, b1=b1, w2=w2, b2=b2, dil=dil, scale=scale, y_prev=y_prev)
    worst = R.check(outs[0][:T], ref, bar, want)
    print(f"[route] pair C{C_} taps{taps} acc{int(acc)} T{T} {routes[0]} worst err/bar {worst:.3f}")


@pytest.mark.parametrize("taps", [1, -1, 13, 2, 4])
def test_conv_pair_refuses_uninstantiated_taps_on_device(taps):
    """valid device buffers, a tap count without a kernel: an error and no launch (the record stays empty)"""
    from gsv import _lib
    _lib.init(0)
    C_, T = 16, 1024
    x = torch.zeros(T, C_, dtype=torch.float16, device=DEV)
    w = torch.zeros(C_, 11 * C_, dtype=torch.float16, device=DEV)
    b = torch.zeros(C_, device=DEV)
    y = _sentinel((T, C_), torch.float16)
    _lib.lib().gsv_debug_last_conv_route(1)
    rc = _lib.lib().gsv_op_conv_pair(x.data_ptr(), w.data_ptr(), b.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), T, C_,
                                     taps, 1, 1.0, 0, None)
    torch.cuda.synchronize()
    assert rc != 0 and _route() == "none"
    assert torch.all(_bits(y) == SENT[torch.float16][1])
