"""What the GPU tests of the loudness meter share: seeded speech-like signals, sentences as misaligned device views, and the calls
gsv_op_loudness / gsv_postprocess_groups_loud over [(sentences, gap)] groups with (first, count, gaps, target, peak_db) spans."""
import ctypes as C
import math

import numpy as np

import _loudness_ref as R


def speech(rng, n, rate, amp=0.3, dc=0.05):
    """a harmonic stack under a slow envelope, a DC offset and a little noise -> fp64 [n]"""
    t = np.arange(n) / float(rate)
    f0 = 110.0 + 80.0 * rng.random()
    stack = sum(np.sin(2 * np.pi * k * f0 * t + 2 * np.pi * rng.random()) / k for k in range(1, 9))
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 3.0 * t + 2 * np.pi * rng.random())
    return amp * env * stack / 1.5 + dc + 0.01 * rng.standard_normal(n)


def views(sentences, dev):
    """each numpy sentence as a view into one device buffer, sentence i starting 1 + i % 7 elements past a 16-byte boundary"""
    import torch
    dt = sentences[0].dtype if sentences else np.dtype(np.float32)
    per = 16 // dt.itemsize
    starts, at = [], 0
    for i, s in enumerate(sentences):
        at = (at + per - 1) // per * per + 1 + i % 7
        starts.append(at)
        at += s.shape[0]
    host = np.zeros(at + per, dtype=dt)
    for s, a in zip(sentences, starts):
        host[a:a + s.shape[0]] = s
    buf = torch.from_numpy(host).to(dev)
    return buf, [buf[a:a + s.shape[0]] for s, a in zip(sentences, starts)]


class Call:
    """the host and device arrays of one call; kept alive until the results are read"""

    def __init__(self, groups, spans, rate, dev):
        import torch
        from gsv import _lib
        self.keep, flat = [], []
        for sents, _ in groups:
            buf, v = views(list(sents), dev)
            self.keep.append(buf)
            flat += v
        self.n, self.ng, self.ns = len(flat), len(groups), len(spans)
        self.code = _lib.dtype_code(flat[0].dtype)
        self.lens = (C.c_int * max(self.n, 1))(*[int(v.numel()) for v in flat])
        self.ptrs = (C.c_void_p * max(self.n, 1))(*[v.data_ptr() for v in flat])
        self.gn = (C.c_int * max(self.ng, 1))(*[len(s) for s, _ in groups])
        self.gg = (C.c_int * max(self.ng, 1))(*[g for _, g in groups])
        self.off = (C.c_longlong * (self.ng + 1))()
        self.spans = (_lib.LoudSpan * max(self.ns, 1))(*[
            _lib.LoudSpan(f, c, int(gaps), float("nan") if tgt is None else tgt, pk) for f, c, gaps, tgt, pk in spans])
        self.rate = rate
        l = _lib.lib()
        need = int(l.gsv_postprocess_groups_loud_workspace(self.lens, self.n, self.gn, self.gg, self.ng, rate if rate > 0 else 32000, self.ns))
        assert need >= 0
        self.table = torch.empty(need + 16, dtype=torch.uint8).pin_memory()
        self.work = torch.empty(need + 16, dtype=torch.uint8, device=dev)
        self.report = torch.zeros(max(self.ns, 1) * 16, dtype=torch.uint8, device=dev)
        self.dev = dev

    def reports(self):
        from gsv import _lib
        return self.report.cpu().numpy().view(_lib.LOUD_REPORT_DTYPE)[:self.ns]


def op_loudness(groups, spans, rate, dev="cuda:0"):
    """gsv_op_loudness -> (energies per span, report records)"""
    import torch
    from gsv import _lib
    c = Call(groups, spans, rate, dev)
    s = int(round(0.1 * rate))
    cap = sum(sum(x.shape[0] + g for x in sents) for sents, g in groups) // s + len(spans) + 1
    en = torch.full((cap,), 7.0, dtype=torch.float64, device=dev)
    eoff = (C.c_longlong * (len(spans) + 1))()
    st = torch.cuda.current_stream()
    _lib.check(_lib.lib().gsv_op_loudness(c.ptrs, c.lens, c.n, c.code, c.gn, c.gg, c.ng, rate, c.spans, c.ns, en.data_ptr(), eoff,
                                         c.report.data_ptr(), c.table.data_ptr(), c.work.data_ptr(), C.c_void_p(st.cuda_stream)),
               "gsv_op_loudness")
    torch.cuda.synchronize()
    en = en.cpu().numpy()
    eoff = [int(o) for o in eoff]
    assert eoff[-1] < cap and (en[eoff[-1]:] == 7.0).all(), "an energy outside the spans' slots was written"
    return [en[eoff[k]:eoff[k + 1]] for k in range(len(spans))], c.reports()


def loud(groups, spans, rate, h, up, down, fmt, dev="cuda:0", shift=1, entry="loud"):
    """gsv_postprocess_groups_loud (entry="rate": gsv_postprocess_groups_rate on the same arguments, the spans ignored)
    -> (one output array per group, report records)"""
    import torch
    from gsv import _lib
    out_dt = {_lib.GSV_OUT_S16: torch.int16, _lib.GSV_OUT_MULAW: torch.uint8, _lib.GSV_OUT_ALAW: torch.uint8,
              _lib.GSV_OUT_F32: torch.float32}[fmt]
    c = Call(groups, spans, rate, dev)
    total = sum((sum(x.shape[0] + g for x in sents) * up + down - 1) // down for sents, g in groups)
    guard = 0x5a if out_dt != torch.float32 else 1234.5
    out = torch.full((total + shift + 1,), guard, dtype=out_dt, device=dev)
    hd = torch.from_numpy(np.ascontiguousarray(h, dtype=np.float32)).to(dev)
    st = torch.cuda.current_stream()
    l = _lib.lib()
    dst = out.data_ptr() + shift * out.element_size()
    if entry == "rate":
        rc = l.gsv_postprocess_groups_rate(c.ptrs, c.lens, c.n, c.code, c.gn, c.gg, c.ng, dst, c.off, c.table.data_ptr(),
                                           c.work.data_ptr(), hd.data_ptr(), int(hd.numel()), up, down, fmt, C.c_void_p(st.cuda_stream))
    else:
        rc = l.gsv_postprocess_groups_loud(c.ptrs, c.lens, c.n, c.code, c.gn, c.gg, c.ng, dst, c.off, c.table.data_ptr(),
                                           c.work.data_ptr(), hd.data_ptr(), int(hd.numel()), up, down, fmt, rate, c.spans, c.ns,
                                           c.report.data_ptr(), C.c_void_p(st.cuda_stream))
    _lib.check(rc, "gsv_postprocess_groups_" + entry)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    off = [int(o) for o in c.off]
    assert off[0] == 0 and off[-1] == total
    assert (got[:shift] == guard).all() and got[-1] == guard, "an element outside the packed buffer was written"
    got = got[shift:-1]
    return [got[off[g]:off[g + 1]] for g in range(len(groups))], c.reports()


def mirror_span(groups, span, rate):
    """the mirror of one span -> (meter dict, gain fp64, flags)"""
    first, count, gaps, target, peak_db = span
    flat = [(x, g) for sents, g in groups for x in sents]
    sents = [x for x, _ in flat[first:first + count]]
    gap = flat[first][1]
    m = R.meter(R.span_stream(sents, gap, gaps), rate)
    g, flags = R.span_gain(m["lufs"], target, peak_db, sents)
    return m, g, flags


def ulps32(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def check_span(en, rep, m, g, flags, worst):
    """the bars of the op test for one span; `worst` collects the largest fractions of the energy and the level bar"""
    assert int(rep["flags"]) == flags, (int(rep["flags"]), flags)
    if flags & R.NAN:
        assert float(rep["gain"]) == 1.0
        return
    assert en.shape == m["energies"].shape
    live = R.level(m["energies"] / m["s"]) > -70.0
    if live.any():
        rel = np.abs(en[live] - m["energies"][live]) / m["energies"][live]
        worst["energy"] = max(worst["energy"], float(rel.max()) / 1e-9)
        assert rel.max() <= 1e-9, rel.max()
    if m["lufs"] == -math.inf:
        assert float(rep["lufs"]) == -math.inf and float(rep["gain"]) == 1.0
    else:
        d = abs(float(rep["lufs"]) - m["lufs"])
        worst["lufs"] = max(worst["lufs"], d / 1e-8)
        assert d <= 1e-8, d
        assert ulps32(rep["gain"], np.float32(g)) <= 1, (float(rep["gain"]), g)
