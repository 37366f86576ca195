"""Every entry point of include/kofft_hip.h inside guard bands (tests/redzone.py): a call writes its outputs and nothing else, and leaves
what the header declares `const` as it found it.  Section 1 runs the device-pointer (`_dev`) forms with every pointer in one arena on
the device, section 2 the host-pointer forms in a numpy arena through raw ctypes calls.  Each case runs its call twice, then
(a) arena.verify(): no byte of a band and no byte of an input changed, (b) every row of every output against the family's oracle, bit
for bit -- the bands hold NaN, so an over-read that reaches a result shows here -- and (c) the two runs gave the same bytes.

The cases are data: DEV_CASES / HOST_CASES, one driver per call signature.  Shapes sit where the last tile or workgroup is ragged:
batch 1, around multiples of 256 (the CU count, the persistent kernels' grid), one length per kernel family.  A case holds at most
2^22 points in + out -- except route="stream": the streaming kernels start at CUs x k rows (host_common.hip.h: launch_persist /
launch_split from batch >= 256 * 4 .. 256 * 32), which at every length but 4096 lies beyond that cap, and a ragged last round of
those persistent grids is what this module is for; they get one batch each, a few rows past the threshold -- and the two host
pipeline cases, which need 128 MiB to take that path.

What the bands do not see: the library's own scratch (real_tmp, the large-n intermediate, the Bluestein work buffer, host staging)
is allocated inside the library and lies outside every arena."""
import ctypes as C_
import re
import zlib
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import pytest

import wavelet_oracle as wo
from cepstrum_oracle import cepstrum_ref
from dct_oracle import dct2_ref
from hilbert_oracle import hilbert_ref
from redzone import Arena, RedzoneError
from rowcheck import assert_rows_equal
from test_gpu_route_coverage import _oracle_axis
from trig_direct_oracle import direct

pytestmark = pytest.mark.gpu

ALIGN_OFFS = (0, 4, 8, 16)  # bytes past a 256-byte boundary: the weakest alignment the header allows per buffer, see _align
MAX_POINTS = 1 << 22

Case = namedtuple("Case", "call dtype n batch route align_off opt")


def K(call, n, batch, route=None, align_off=0, **opt):
    dtype = re.search(r"(c32|c64|f32|f64)", call).group(1)
    assert align_off in ALIGN_OFFS
    return Case(call, dtype, n, batch, route, align_off, tuple(sorted(opt.items())))


def case_id(c):
    opt = "".join(f"-{k}={v}" for k, v in c.opt)
    return f"{c.call}-n{c.n}-b{c.batch}-{c.route or 'default'}-a{c.align_off}{opt}"


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------
def _real(dtype):
    return np.float64 if dtype in ("c64", "f64") else np.float32


def _cplx(dtype):
    return np.complex128 if dtype in ("c64", "f64") else np.complex64


def _rng(c):
    return np.random.default_rng(zlib.crc32(case_id(c).encode()))


def _rr(rng, shape, dtype=np.float32):
    return rng.uniform(-1, 1, shape).astype(dtype)


def _rc(rng, shape, cdt=np.complex64):
    real = np.float32 if cdt == np.complex64 else np.float64
    return (rng.uniform(-1, 1, shape).astype(real) + 1j * rng.uniform(-1, 1, shape).astype(real)).astype(cdt)


def _p(region):
    return None if region is None else C_.c_void_p(region.addr)


def _setup(E, c, dev):
    """(context wrapper, C function, arena) of a case."""
    f = E.f64 if c.dtype in ("c64", "f64") else E.f32
    return f, getattr(f._lib, "kofft_hip_" + c.call), Arena("cuda" if dev else "host", case_id(c))


def _go(c, arena, f, call, outs, restore=(), nan_safe=False):
    """Run `call` twice (the buffers in `restore` put back in between), then bands and inputs, then every output (region, dtype,
    shape, want, label) against `want` row by row, then run 1 against run 2."""
    what = case_id(c)

    def once():
        f._check(call())
        f.synchronize()
        return [arena.read(r, dt, shape) for r, dt, shape, _, _ in outs]

    first = once()
    for r in restore:
        arena.restore(r)
    second = once()
    arena.verify(what)
    for (r, dt, shape, want, label), a, b in zip(outs, first, second):
        assert_rows_equal(a, np.asarray(want).reshape(shape), f"{what} {label}", nan_safe=nan_safe)
        assert a.tobytes() == b.tobytes(), f"{what} {label}: two runs of the same call differ"


def _plan_ifft_reference(x, forward):
    """FftPlan::ifft (fft.rs:2040-2055) around `forward`: conj, fft, conj * 1/(n as f32 -> T), as test_gpu_parity.py restates it."""
    real = np.float32 if x.dtype == np.complex64 else np.float64
    y = forward(np.conj(x))
    scale = real(1) / real(np.float32(x.shape[-1]))
    out = np.empty_like(y)
    out.real = y.real * scale
    out.imag = (-y.imag) * scale
    return out


# ---- drivers: one per call signature, shared by the device and the host forms where the arguments are the same ---------------------
def drv_fft_inplace(E, c, dev):
    f, fn, arena = _setup(E, c, dev)
    o = dict(c.opt)
    inv = int(o.get("inverse", 0))
    x = _rc(_rng(c), (c.batch, c.n), _cplx(c.dtype))
    d = arena.inout(x, c.align_off, row_bytes=x.itemsize * c.n, name="data")
    _go(c, arena, f, lambda: fn(f._ctx, _p(d), c.n, c.batch, inv), [(d, x.dtype, x.shape, E.oracle.fft_mt(x, inverse=bool(inv)), "data")],
        restore=(d,))


def drv_fft_oop(E, c, dev):
    f, fn, arena = _setup(E, c, dev)
    o = dict(c.opt)
    inv = int(o.get("inverse", 0))
    x = _rc(_rng(c), (c.batch, c.n), _cplx(c.dtype))
    want = E.oracle.fft_mt(x, inverse=bool(inv))
    row = x.itemsize * c.n
    if o.get("same"):  # d_in == d_out is allowed
        d = arena.inout(x, c.align_off, row_bytes=row, name="data")
        _go(c, arena, f, lambda: fn(f._ctx, _p(d), _p(d), c.n, c.batch, inv), [(d, x.dtype, x.shape, want, "data")], restore=(d,))
        return
    i = arena.input(x, c.align_off, row_bytes=row, name="in")
    out = arena.output(x.nbytes, c.align_off, row_bytes=row, name="out")
    _go(c, arena, f, lambda: fn(f._ctx, _p(i), _p(out), c.n, c.batch, inv), [(out, x.dtype, x.shape, want, "out")])


def drv_radix4(E, c, dev):
    f, fn, arena = _setup(E, c, dev)
    x = _rc(_rng(c), (c.batch, c.n), _cplx(c.dtype))
    pow4 = c.n & (c.n - 1) == 0 and (c.n.bit_length() - 1) % 2 == 0
    if c.call.startswith("ifft"):
        want = _plan_ifft_reference(x, E.oracle.fft_radix4) if pow4 else E.oracle.fft_mt(x, inverse=True)
    else:
        want = E.oracle.fft_radix4(x)
    row = x.itemsize * c.n
    i = arena.input(x, c.align_off, row_bytes=row, name="in")
    out = arena.output(x.nbytes, c.align_off, row_bytes=row, name="out")
    _go(c, arena, f, lambda: fn(f._ctx, _p(i), _p(out), c.n, c.batch), [(out, x.dtype, x.shape, want, "out")])


def drv_rfft(E, c, dev):
    f, fn, arena = _setup(E, c, dev)
    rng = _rng(c)
    rdt, cdt = _real(c.dtype), _cplx(c.dtype)
    x = _rr(rng, (c.batch, c.n), rdt)
    win = rng.uniform(0.1, 1, c.n).astype(rdt) if dict(c.opt).get("window") else None
    m1 = c.n // 2 + 1
    i = arena.input(x, c.align_off, row_bytes=x.itemsize * c.n, name="in")
    w = None if win is None else arena.input(win, c.align_off, name="window")
    # complex rows of n/2 + 1: an odd row length, at the weakest alignment of a complex value
    out = arena.output(c.batch * m1 * 2 * x.itemsize, 2 * c.align_off if c.align_off in (4, 8) else c.align_off, row_bytes=m1 * 2 * x.itemsize, name="out")
    _go(c, arena, f, lambda: fn(f._ctx, _p(i), _p(out), _p(w), c.n, c.batch), [(out, cdt, (c.batch, m1), E.oracle.rfft_mt(x, win), "out")])


def drv_irfft(E, c, dev):
    f, fn, arena = _setup(E, c, dev)
    rdt = _real(c.dtype)
    x = E.oracle.rfft_mt(_rr(_rng(c), (c.batch, c.n), rdt))
    m1 = c.n // 2 + 1
    i = arena.input(x, 2 * c.align_off if c.align_off in (4, 8) else c.align_off, row_bytes=x.itemsize * m1, name="in")
    out = arena.output(c.batch * c.n * np.dtype(rdt).itemsize, c.align_off, row_bytes=c.n * np.dtype(rdt).itemsize, name="out")
    _go(c, arena, f, lambda: fn(f._ctx, _p(i), _p(out), c.n, c.batch), [(out, rdt, (c.batch, c.n), E.oracle.irfft_mt(x, c.n), "out")])


ROWWISE = {"dct2": (dct2_ref, "set_dct_fused", np.float32), "hilbert": (hilbert_ref, "set_hilbert_fused", np.complex64),
           "cepstrum": (cepstrum_ref, "set_cepstrum_fused", np.float32)}


def drv_rowwise(E, c, dev):
    """dct2 / hilbert / cepstrum: (ctx, in, out, n, batch); route fused / composed."""
    f, fn, arena = _setup(E, c, dev)
    ref, setter, odt = ROWWISE[c.call.split("_")[0]]
    x = _rr(_rng(c), (c.batch, c.n))
    with np.errstate(all="ignore"):
        want = ref(x)
    getattr(f, setter)(c.route != "composed")
    try:
        if dict(c.opt).get("same"):  # cepstrum: in == out
            d = arena.inout(x, c.align_off, row_bytes=4 * c.n, name="data")
            _go(c, arena, f, lambda: fn(f._ctx, _p(d), _p(d), c.n, c.batch), [(d, odt, x.shape, want, "data")], restore=(d,), nan_safe=True)
            return
        i = arena.input(x, c.align_off, row_bytes=4 * c.n, name="in")
        osz = np.dtype(odt).itemsize
        # the analytic signal's complex output must be 8-byte aligned: only its input sits at +4
        out = arena.output(c.batch * c.n * osz, 8 if (osz == 8 and c.align_off) else c.align_off, row_bytes=c.n * osz, name="out")
        _go(c, arena, f, lambda: fn(f._ctx, _p(i), _p(out), c.n, c.batch), [(out, odt, x.shape, want, "out")], nan_safe=True)
    finally:
        getattr(f, setter)(True)


def drv_direct(E, c, dev):
    f, fn, arena = _setup(E, c, dev)
    o = dict(c.opt)
    fam, t = c.call[:3], int(o["type"])
    x = _rr(_rng(c), (c.batch, c.n))
    want = direct(fam, t, x) if c.n <= 64 else E.oracle.direct_mt(fam, t, x)
    f.set_direct_tiled(c.route != "simple")
    try:
        if o.get("same"):  # host form only
            d = arena.inout(x, c.align_off, row_bytes=4 * c.n, name="data")
            _go(c, arena, f, lambda: fn(f._ctx, t, _p(d), _p(d), c.n, c.batch), [(d, np.float32, x.shape, want, "data")], restore=(d,), nan_safe=True)
            return
        i = arena.input(x, c.align_off, row_bytes=4 * c.n, name="in")
        out = arena.output(x.nbytes, c.align_off, row_bytes=4 * c.n, name="out")
        _go(c, arena, f, lambda: fn(f._ctx, t, _p(i), _p(out), c.n, c.batch), [(out, np.float32, x.shape, want, "out")], nan_safe=True)
    finally:
        f.set_direct_tiled(True)


def drv_dwt(E, c, dev):
    f, fn, arena = _setup(E, c, dev)
    name = dict(c.opt)["wavelet"]
    x = _rr(_rng(c), (c.batch, c.n))
    h = c.n // 2  # an odd length writes len / 2; len == 1 writes nothing at all
    wa, wd = wo.forward(name, x)
    i = arena.input(x, c.align_off, row_bytes=4 * c.n, name="in")
    a = arena.output(4 * c.batch * h, c.align_off, row_bytes=4 * h, name="approx")
    d = arena.output(4 * c.batch * h, c.align_off, row_bytes=4 * h, name="detail")
    _go(c, arena, f, lambda: fn(f._ctx, wo.NAMES.index(name), _p(i), _p(a), _p(d), c.n, c.batch),
        [(a, np.float32, (c.batch, h), wa, "approx"), (d, np.float32, (c.batch, h), wd, "detail")], nan_safe=True)


def drv_idwt(E, c, dev):
    f, fn, arena = _setup(E, c, dev)
    name = dict(c.opt)["wavelet"]
    rng = _rng(c)
    ap, dt = _rr(rng, (c.batch, c.n)), _rr(rng, (c.batch, c.n))
    a = arena.input(ap, c.align_off, row_bytes=4 * c.n, name="approx")
    d = arena.input(dt, c.align_off, row_bytes=4 * c.n, name="detail")
    out = arena.output(8 * c.batch * c.n, c.align_off, row_bytes=8 * c.n, name="out")
    _go(c, arena, f, lambda: fn(f._ctx, wo.NAMES.index(name), _p(a), _p(d), _p(out), c.n, c.batch),
        [(out, np.float32, (c.batch, 2 * c.n), wo.inverse(name, ap, dt), "out")], nan_safe=True)


def _wavelet_route(f, c):
    f.set_wavelet_fused({"level": 0, "fused": 2}.get(c.route, 1))


def drv_dwt_multi(E, c, dev, short_rows=0):
    """`short_rows`: the sensitivity check tells the arena that approx holds that many rows fewer than the call writes."""
    f, fn, arena = _setup(E, c, dev)
    o = dict(c.opt)
    name, levels = o["wavelet"], int(o["levels"])
    x = _rr(_rng(c), (c.batch, c.n))
    lens = wo.multi_lengths(c.n, levels)
    got_lens = (C_.c_size_t * (levels + 1))()
    assert f._lib.kofft_hip_dwt_multi_lengths(c.n, levels, got_lens) == 0 and list(got_lens) == lens
    wa, wds = wo.forward_multi(name, x, levels)
    i = arena.input(x, c.align_off, row_bytes=4 * c.n, name="in")
    a = arena.output(4 * (c.batch - short_rows) * lens[-1], c.align_off, row_bytes=4 * lens[-1], name="approx")
    tot = c.batch * sum(lens[1:])  # exactly the packed size: the band starts right behind it
    d = arena.output(4 * tot, c.align_off, row_bytes=4 * lens[1], name="details") if levels else None  # levels == 0: details may be null
    outs = [] if short_rows else [(a, np.float32, (c.batch, lens[-1]), wa, "approx")]
    if levels:
        outs.append((d, np.float32, (tot,), np.concatenate([w.ravel() for w in wds]), "details (packed)"))
    _wavelet_route(f, c)
    try:
        _go(c, arena, f, lambda: fn(f._ctx, wo.NAMES.index(name), _p(i), _p(a), _p(d), c.n, c.batch, levels), outs, nan_safe=True)
    finally:
        f.set_wavelet_fused(1)


def drv_idwt_multi(E, c, dev):
    f, fn, arena = _setup(E, c, dev)
    o = dict(c.opt)
    name, levels, longer = o["wavelet"], int(o["levels"]), int(o.get("longer", 0))
    rng = _rng(c)
    n0 = c.n
    dl = [(n0 << (levels - 1 - l)) + longer for l in range(levels)]  # detail rows one longer than what is read
    ap = _rr(rng, (c.batch, n0))
    dets = [_rr(rng, (c.batch, m)) for m in dl]
    a = arena.input(ap, c.align_off, row_bytes=4 * n0, name="approx")
    d = arena.input(np.concatenate([v.ravel() for v in dets]), c.align_off, row_bytes=4 * dl[0], name="details") if levels else None
    total = n0 << levels
    out = arena.output(4 * c.batch * total, c.align_off, row_bytes=4 * total, name="out")
    lens = (C_.c_size_t * max(1, levels))(*dl)
    _wavelet_route(f, c)
    try:
        _go(c, arena, f, lambda: fn(f._ctx, wo.NAMES.index(name), _p(a), _p(d), lens, _p(out), n0, c.batch, levels),
            [(out, np.float32, (c.batch, total), wo.inverse_multi(name, ap, dets), "out")], nan_safe=True)
    finally:
        f.set_wavelet_fused(1)


def _stft_signal(c, rng, first, count, hop):
    """A signal that ends inside the third frame from the end: the last frames are partly and wholly past it."""
    total = max(1, (first + count - 3) * hop + c.n // 3)
    return _rr(rng, (total,))


def drv_stft_dev(E, c, dev):
    """n = win_len, batch = count; opt hop, first."""
    f, fn, arena = _setup(E, c, dev)
    o = dict(c.opt)
    hop, first = int(o["hop"]), int(o.get("first", 0))
    rng = _rng(c)
    sig = _stft_signal(c, rng, first, c.batch, hop)
    win = rng.uniform(0.1, 1, c.n).astype(np.float32)
    s = arena.input(sig, c.align_off, name="signal")
    w = arena.input(win, c.align_off, name="window")
    out = arena.output(8 * c.batch * c.n, 0, row_bytes=8 * c.n, name="out")
    _go(c, arena, f, lambda: fn(f._ctx, _p(s), sig.size, _p(w), c.n, hop, _p(out), first, c.batch),
        [(out, np.complex64, (c.batch, c.n), E.oracle.stft_range(sig, win, hop, first, c.batch), "out")])


def drv_stft_host(E, c, dev):
    """stft (frames >= ceil(len / hop), some wholly past the end) and stft_parallel (any frame count, here fewer)."""
    f, fn, arena = _setup(E, c, dev)
    hop = int(dict(c.opt)["hop"])
    rng = _rng(c)
    sig = _stft_signal(c, rng, 0, c.batch, hop) if "parallel" not in c.call else _rr(rng, ((c.batch + 5) * hop,))
    win = rng.uniform(0.1, 1, c.n).astype(np.float32)
    s = arena.input(sig, c.align_off, name="signal")
    w = arena.input(win, c.align_off, name="window")
    out = arena.output(8 * c.batch * c.n, 0, row_bytes=8 * c.n, name="out")
    _go(c, arena, f, lambda: fn(f._ctx, _p(s), sig.size, _p(w), c.n, hop, _p(out), c.batch),
        [(out, np.complex64, (c.batch, c.n), E.oracle.stft_range(sig, win, hop, 0, c.batch), "out")])


def drv_stft_frame(E, c, dev):
    f, fn, arena = _setup(E, c, dev)
    start = int(dict(c.opt)["start"])
    rng = _rng(c)
    sig = _rr(rng, (start + c.n // 2,))  # the frame runs past the end
    win = rng.uniform(0.1, 1, c.n).astype(np.float32)
    s = arena.input(sig, c.align_off, name="signal")
    w = arena.input(win, c.align_off, name="window")
    out = arena.output(8 * c.n, 0, name="frame_out")
    _go(c, arena, f, lambda: fn(f._ctx, _p(s), sig.size, _p(w), c.n, start, _p(out)),
        [(out, np.complex64, (1, c.n), E.oracle.stft_range(sig, win, start, 1, 1), "frame_out")])


def _oracle_istft(E, spec, win, hop, pre):
    """stft::istft accumulating into `pre`: (output, scratch), through the oracle's C entry as test_istft_reference_tests does."""
    fr, out, scr = spec.copy(), pre.copy(), np.zeros(pre.size, np.float32)
    v, z = C_.c_void_p, C_.c_size_t
    rc = E.oracle.lib().ko_istft_f32(v(fr.ctypes.data), z(fr.shape[0]), v(win.ctypes.data), z(win.size), z(hop), v(out.ctypes.data), z(out.size),
                                     v(scr.ctypes.data), z(scr.size))
    assert rc == 0
    return out, scr


def drv_istft(E, c, dev):
    """n = win_len, batch = frames; opt hop, delta (out_len relative to what the frames reach).  d_frames is modified by contract
    (the inverse transforms), d_output accumulates, d_scratch receives the window-square sums."""
    f, fn, arena = _setup(E, c, dev)
    o = dict(c.opt)
    hop = int(o["hop"])
    out_len = (c.batch - 1) * hop + c.n + int(o.get("delta", 0))
    rng = _rng(c)
    spec = _rc(rng, (c.batch, c.n))
    win = (E.oracle.hann(c.n) + np.float32(0.01)).astype(np.float32)
    pre = _rr(rng, (out_len,))
    want, want_scr = _oracle_istft(E, spec, win, hop, pre)
    fr = arena.inout(spec, 8 if c.align_off else 0, row_bytes=8 * c.n, name="frames")
    w = arena.input(win, c.align_off, name="window")
    out = arena.output(4 * out_len, c.align_off, prefill=pre, row_bytes=4 * hop, name="output")
    scr = arena.output(4 * out_len, c.align_off, row_bytes=4 * hop, name="scratch")
    _go(c, arena, f, lambda: fn(f._ctx, _p(fr), c.batch, _p(w), c.n, hop, _p(out), out_len, _p(scr), out_len),
        [(out, np.float32, (out_len,), want, "output"), (scr, np.float32, (out_len,), want_scr, "scratch"),
         (fr, np.complex64, spec.shape, E.oracle.fft_mt(spec, inverse=True), "frames left behind")], restore=(fr, out))


def drv_istft_parallel(E, c, dev):
    """Host only: the frames are not modified; samples whose window-square sum is <= 1e-8 are set to 0."""
    f, fn, arena = _setup(E, c, dev)
    hop = int(dict(c.opt)["hop"])
    out_len = (c.batch - 1) * hop + c.n + int(dict(c.opt).get("delta", 0))
    spec = _rc(_rng(c), (c.batch, c.n))
    win = E.oracle.hann(c.n)
    want, scr = _oracle_istft(E, spec, win, hop, np.zeros(out_len, np.float32))
    want[scr <= 1e-8] = 0.0
    fr = arena.input(spec, c.align_off, row_bytes=8 * c.n, name="frames")
    w = arena.input(win, c.align_off, name="window")
    out = arena.output(4 * out_len, c.align_off, prefill=np.zeros(out_len, np.float32), row_bytes=4 * hop, name="output")
    _go(c, arena, f, lambda: fn(f._ctx, _p(fr), c.batch, _p(w), c.n, hop, _p(out), out_len), [(out, np.float32, (out_len,), want, "output")],
        restore=(out,))


def drv_istft_frame(E, c, dev):
    """Host only: ifft(frame) in place, then output[start + i] += frame[i].re * window[i] for start + i < out_len."""
    f, fn, arena = _setup(E, c, dev)
    start = int(dict(c.opt)["start"])
    out_len = start + c.n // 2  # the frame runs past the end of the output
    rng = _rng(c)
    frame = _rc(rng, (1, c.n))
    win = rng.uniform(0.1, 1, c.n).astype(np.float32)
    pre = _rr(rng, (out_len,))
    time = E.oracle.fft(frame, inverse=True)
    want = pre.copy()
    k = out_len - start
    want[start:] = pre[start:] + time[0, :k].real * win[:k]
    fr = arena.inout(frame, c.align_off, name="frame")
    w = arena.input(win, c.align_off, name="window")
    out = arena.output(4 * out_len, c.align_off, prefill=pre, name="output")
    _go(c, arena, f, lambda: fn(f._ctx, _p(fr), _p(w), c.n, start, _p(out), out_len),
        [(out, np.float32, (out_len,), want, "output"), (fr, np.complex64, (1, c.n), time, "frame left behind")], restore=(fr, out))


def drv_magnitudes(E, c, dev):
    """n = win_len, batch = frames = ceil(len / hop); d_max is a single float inside bands."""
    f, fn, arena = _setup(E, c, dev)
    hop = int(dict(c.opt)["hop"])
    sig = _rr(_rng(c), (c.batch * hop - hop // 2,))
    wm, wmax = E.oracle.stft_magnitudes(sig, c.n, hop)
    assert wm.shape == (c.batch, c.n // 2)
    s = arena.input(sig, c.align_off, name="samples")
    m = arena.output(wm.nbytes, c.align_off, row_bytes=4 * (c.n // 2), name="mags")
    mx = arena.output(4, c.align_off, name="max")
    _go(c, arena, f, lambda: fn(f._ctx, _p(s), sig.size, c.n, hop, _p(m), c.batch, _p(mx)),
        [(m, np.float32, wm.shape, wm, "mags"), (mx, np.float32, (1,), np.array([wmax], np.float32), "max")])


def drv_fftnd(E, c, dev):
    """n = cols, batch = rows; opt depth, inverse."""
    f, fn, arena = _setup(E, c, dev)
    o = dict(c.opt)
    depth, inv = int(o.get("depth", 1)), bool(o.get("inverse", 0))
    x = _rc(_rng(c), (depth, c.batch, c.n), _cplx(c.dtype))
    want = x
    for axis in ((0, 1, 2) if depth > 1 else (2, 1)):  # ndfft.rs:114-155 / 74-101
        want = _oracle_axis(E.oracle, want, axis, inv)
    d = arena.inout(x, c.align_off, row_bytes=x.itemsize * c.n, name="data")
    _go(c, arena, f, lambda: fn(f._ctx, _p(d), depth, c.batch, c.n, int(inv)), [(d, x.dtype, x.shape, want, "data")], restore=(d,))


def drv_strided(E, c, dev):
    """Host only: n elements data[i * stride] transformed; the elements between them and behind the last keep their bytes."""
    f, fn, arena = _setup(E, c, dev)
    o = dict(c.opt)
    stride, inv = int(o["stride"]), int(o.get("inverse", 0))
    data_len = (c.n - 1) * stride + 1 + int(o.get("slack", 0))
    buf = _rc(_rng(c), (data_len,), _cplx(c.dtype))
    want = buf.copy()
    want[::stride][:c.n] = E.oracle.fft(buf[::stride][:c.n][None], inverse=bool(inv))[0]
    d = arena.inout(buf, c.align_off, name="data")
    _go(c, arena, f, lambda: fn(f._ctx, _p(d), data_len, stride, c.n, inv), [(d, buf.dtype, buf.shape, want, "data")], restore=(d,))


# ---- the cases --------------------------------------------------------------------------------------------------------------------
WAVELETS = wo.NAMES
AROUND_CUS = (255, 256, 257)


def _dev_cases():
    cs = []
    # complex, in place: one length per kernel family; batch 1, around the CU count, the cap
    for n, batches in ((64, (1, 255, 257, 4097)), (512, (1, 257, 1025)), (1024, (1, 255, 257)), (2048, (1, 257, 2047)), (4096, (1, 255, 256, 257, 1023, 1024)),
                       (8192, (1, 257, 511)), (16384, (1, 3, 255)), (32768, (1, 127)), (1000, (1, 257, 2049)), (6000, (1, 5, 300))):
        for k, b in enumerate(batches):
            cs.append(K("fft_c32_dev", n, b, align_off=8 if k % 2 else 0, inverse=k % 2))
    for n, batches in ((64, (1, 257)), (1024, (1, 257)), (4096, (1, 255, 513)), (8192, (1, 255)), (16384, (1, 127, 255)), (1000, (1, 257))):
        for k, b in enumerate(batches):
            cs.append(K("fft_c64_dev", n, b, align_off=16 if k % 2 else 0, inverse=(k + 1) % 2))
    # two factor kernels through the intermediate: one transform, a mid step of the ladder, the persistent factor kernels
    cs += [K("fft_c32_dev", 1 << 15, b, inverse=b == 17) for b in (1, 17, 127, 128)]
    cs += [K("fft_c64_dev", 1 << 15, b, inverse=b == 17) for b in (1, 17, 127)]
    # the streaming kernels' ragged last round (beyond the cap, see the module docstring)
    cs += [K("fft_c32_dev", n, b, "stream", inverse=n == 2048) for n, b in ((512, 16387), (1024, 8195), (2048, 4099), (4096, 1031), (4096, 1500), (8192, 1031), (32768, 515))]
    cs += [K("fft_c64_dev", n, b, "stream") for n, b in ((4096, 2051), (16384, 515))]
    # out of place, and d_in == d_out
    for n, batches in ((64, (1, 257)), (1024, (255, 257)), (4096, (1, 255, 257, 511)), (8192, (129,)), (16384, (1, 127)), (1000, (257,)), (1 << 15, (1, 17, 63))):
        for k, b in enumerate(batches):
            cs.append(K("fft_c32_dev_oop", n, b, align_off=8 if k % 2 else 0, inverse=k % 2))
    cs += [K("fft_c32_dev_oop", 4096, 257, same=1), K("fft_c32_dev_oop", 1 << 15, 17, same=1), K("fft_c32_dev_oop", 4096, 1031, "stream")]
    for n, batches in ((64, (257,)), (4096, (1, 255)), (16384, (1, 63)), (1000, (257,)), (1 << 15, (17,))):
        for k, b in enumerate(batches):
            cs.append(K("fft_c64_dev_oop", n, b, align_off=16 if k % 2 else 0, inverse=k % 2))
    cs += [K("fft_c64_dev_oop", 4096, 255, same=1)]
    # the reference's radix-4 arm: powers of four and not
    for call in ("fft_radix4_c32_dev", "ifft_radix4_c32_dev", "fft_radix4_c64_dev", "ifft_radix4_c64_dev"):
        a = 8 if "c32" in call else 16
        cs += [K(call, 1024, 257, align_off=a), K(call, 4096, 1), K(call, 65536, 3), K(call, 2048, 255), K(call, 12, 257, align_off=a)]
    # real transforms: rows of n/2 + 1 complex out / in
    for call in ("rfft_f32_dev", "rfft_f64_dev"):
        a = 4 if "f32" in call else 8
        for n, batches in ((64, (1, 257)), (1024, (255, 257)), (2048, (1, 257, 1023)), (4096, (255, 511)), (8192, (1, 255)), (16384, (1, 127)), (32768, (63,)), (1000, (257,))):
            for k, b in enumerate(batches):
                cs.append(K(call, n, b, align_off=a if k % 2 == 0 else 0, window=k % 2))
    cs += [K("rfft_f32_dev", 2048, 8300, "stream", align_off=4, window=1), K("rfft_f32_dev", 4096, 4200, "stream"), K("rfft_f64_dev", 4096, 4099, "stream", window=1)]
    for call in ("irfft_f32_dev", "irfft_f64_dev"):
        a = 4 if "f32" in call else 8
        for n, batches in ((64, (1, 257)), (1024, (255, 257)), (2048, (1, 1023)), (4096, (257,)), (8192, (255,)), (16384, (1, 127)), (1000, (257,))):
            for k, b in enumerate(batches):
                cs.append(K(call, n, b, align_off=a if k % 2 == 0 else 0))
    cs += [K("irfft_f32_dev", 2048, 8300, "stream", align_off=4), K("irfft_f64_dev", 4096, 4099, "stream")]
    # DCT-II, analytic signal, cepstrum: fused and composed
    for call, a_fused in (("dct2_f32_dev", 8), ("hilbert_f32_dev", 4), ("cepstrum_f32_dev", 4)):
        for route in ("fused", "composed"):
            a = a_fused if route == "fused" else 4
            cs += [K(call, 32, 257, route, a), K(call, 1024, 255, route), K(call, 1024, 257, route, a), K(call, 4096, 1, route, a), K(call, 4096, 255, route),
                   K(call, 8192, 3, route, a)]
        if call == "dct2_f32_dev":
            cs += [K(call, 1000, 257, "composed", 4), K(call, 63, 255, "composed", 4), K(call, 6000, 5, "fused")]
        if call == "cepstrum_f32_dev":
            cs += [K(call, 1024, 257, "fused", 4, same=1), K(call, 1024, 257, "composed", 4, same=1), K(call, 8192, 3, "fused", same=1)]
    # direct DCT / DST I..IV around the tile edges
    for call in ("dct_direct_f32_dev", "dst_direct_f32_dev"):
        for t in (1, 2, 3, 4):
            for route in ("tiled", "simple"):
                ns = (63, 64, 65, 127, 128, 129)
                n = ns[(t * 2 + (route == "simple") + (call[1] == "s")) % 6]
                cs += [K(call, n, 129, route, 4, type=t), K(call, ns[(t + 3) % 6], 1, route, type=t), K(call, ns[(t + 4) % 6], 63, route, 4, type=t)]
    # wavelets, one level: odd lengths write len / 2, len == 1 nothing
    for k, name in enumerate(WAVELETS):
        cs += [K("dwt_f32_dev", 1, 7, wavelet=name), K("dwt_f32_dev", 1023, 257, align_off=4, wavelet=name), K("dwt_f32_dev", 4096, 255, wavelet=name),
               K("dwt_f32_dev", (3, 9, 17, 33, 5)[k], 1025, align_off=4, wavelet=name),
               K("idwt_f32_dev", 1, 9, wavelet=name), K("idwt_f32_dev", 511, 257, align_off=4, wavelet=name), K("idwt_f32_dev", 2048, 255, wavelet=name)]
    # wavelets, multi level: level by level and fused, odd intermediate lengths, levels == 0
    for k, name in enumerate(WAVELETS):
        for route in ("level", "fused"):
            cs += [K("dwt_multi_f32_dev", 1000, 257, route, 4, wavelet=name, levels=4), K("dwt_multi_f32_dev", (37, 100, 333, 77, 201)[k], 1023, route, wavelet=name, levels=3),
                   K("dwt_multi_f32_dev", 16384, 9, route, wavelet=name, levels=14), K("dwt_multi_f32_dev", 4099, 1, route, 4, wavelet=name, levels=2),
                   K("idwt_multi_f32_dev", 125, 65, route, 4, wavelet=name, levels=3, longer=1), K("idwt_multi_f32_dev", (5, 9, 3, 7, 11)[k], 255, route, wavelet=name, levels=2),
                   K("idwt_multi_f32_dev", 1024, 9, route, wavelet=name, levels=4, longer=1)]
        cs += [K("dwt_multi_f32_dev", 513, 17, "level", 4, wavelet=name, levels=0), K("idwt_multi_f32_dev", 513, 17, "level", 4, wavelet=name, levels=0)]
    cs += [K("dwt_multi_f32_dev", 16385, 5, "fused", wavelet="db4", levels=3)]  # one sample past the fused kernels' row
    # STFT family
    for win, hop in ((1024, 256), (64, 16), (4096, 1024), (1000, 250), (12, 5)):
        cs += [K("stft_f32_dev", win, 37, align_off=4, hop=hop, first=0), K("stft_f32_dev", win, 257, hop=hop, first=11), K("stft_f32_dev", win, 513, align_off=4, hop=hop, first=3)]
    cs += [K("stft_f32_dev", 1024, 8197, "stream", align_off=4, hop=256, first=5)]
    for win, hop in ((1024, 256), (64, 16), (1000, 250), (4096, 4096)):
        for delta in (0, 77, -101 if win > 64 else -9):
            cs.append(K("istft_f32_dev", win, 37 if delta else 258, align_off=4 if delta else 0, hop=hop, delta=delta))
    cs += [K("istft_f32_dev", 1024, 9003, "stream", hop=256, delta=1500), K("istft_f32_dev", 1024, 9000, "stream", align_off=4, hop=256, delta=-777)]
    for win, hop in ((1024, 256), (64, 16), (4096, 1024), (8, 2)):
        cs += [K("stft_magnitudes_f32_dev", win, 37, align_off=4, hop=hop), K("stft_magnitudes_f32_dev", win, 600 if win > 1024 else 2051, hop=hop)]
    # 2-D / 3-D: the fused two-pass sizes (rows >= 1024, cols 1024 / 2048 / 4096, at least 2^22 points), the strided column kernel, others
    for call in ("fftnd_c32_dev", "fftnd_c64_dev"):
        a = 8 if "c32" in call else 16
        cs += [K(call, 1024, 4096, "fused", inverse=0), K(call, 2048, 2048, "fused", inverse=1),
               K(call, 24, 128, align_off=a), K(call, 4, 8192, inverse=1), K(call, 40, 512, align_off=a), K(call, 10, 12), K(call, 6, 100, inverse=1),
               K(call, 7, 5, depth=6, align_off=a), K(call, 16, 1000, depth=2, inverse=1), K(call, 64, 32, depth=16)]
    return cs


def _host_cases():
    """One zero-copy-sized case (each direction at most 512 KiB) and one staged case per host entry point, two pipelined ones."""
    cs = []
    for call, a in (("fft_c32", 8), ("fft_c64", 16)):
        cs += [K(call, 1024, 7, "zero-copy", a), K(call, 4096, 257, "staged", a, inverse=1), K(call, 1000, 129, "staged")]
    cs += [K("fft_c32_strided", 1024, 1, "zero-copy", 8, stride=3, slack=5), K("fft_c32_strided", 8192, 1, "staged", stride=17, slack=100, inverse=1),
           K("fft_c64_strided", 512, 1, "zero-copy", 16, stride=2, slack=1, inverse=1), K("fft_c64_strided", 8192, 1, "staged", stride=9, slack=33)]
    for call, a in (("rfft_f32", 4), ("rfft_f64", 8)):
        cs += [K(call, 1024, 9, "zero-copy", a, window=1), K(call, 2048, 257, "staged", a, window=0), K(call, 4096, 255, "staged", window=1)]
    for call, a in (("irfft_f32", 4), ("irfft_f64", 8)):
        cs += [K(call, 1024, 9, "zero-copy", a), K(call, 2048, 257, "staged", a)]
    for call in ("dct2_f32", "hilbert_f32", "cepstrum_f32"):
        cs += [K(call, 1024, 9, "fused", 4), K(call, 1024, 513, "fused", 4), K(call, 8192, 65, "composed")]
    cs += [K("cepstrum_f32", 1024, 9, "fused", 4, same=1), K("cepstrum_f32", 1024, 513, "composed", same=1)]
    for call in ("dct_direct_f32", "dst_direct_f32"):
        cs += [K(call, 65, 9, "tiled", 4, type=2), K(call, 129, 2049, "tiled", type=3), K(call, 127, 9, "simple", 4, type=1, same=1), K(call, 128, 2049, "tiled", type=4, same=1)]
    cs += [K("dwt_f32", 1023, 9, align_off=4, wavelet="db2"), K("dwt_f32", 4096, 257, wavelet="sym4"),
           K("idwt_f32", 511, 9, align_off=4, wavelet="coif1"), K("idwt_f32", 2048, 257, wavelet="haar"),
           K("dwt_multi_f32", 1000, 9, "fused", 4, wavelet="db4", levels=4), K("dwt_multi_f32", 1000, 513, "level", wavelet="db2", levels=3),
           K("idwt_multi_f32", 125, 9, "fused", 4, wavelet="sym4", levels=3, longer=1), K("idwt_multi_f32", 125, 513, "level", wavelet="haar", levels=3)]
    cs += [K("stft_f32", 1024, 37, "zero-copy", 4, hop=256), K("stft_f32", 1024, 2051, "staged", hop=256),
           K("stft_parallel_f32", 1024, 37, "zero-copy", 4, hop=256), K("stft_parallel_f32", 1000, 2051, "staged", hop=250),
           K("stft_frame_f32", 1024, 1, "zero-copy", 4, start=777), K("stft_frame_f32", 1000, 1, "staged", start=300_001),
           K("istft_f32", 1024, 37, "zero-copy", 4, hop=256, delta=77), K("istft_f32", 1024, 2051, "staged", hop=256, delta=-101),
           K("istft_parallel_f32", 1024, 37, "zero-copy", 4, hop=256, delta=77), K("istft_parallel_f32", 1024, 2051, "staged", hop=256, delta=-101),
           K("istft_frame_f32", 1024, 1, "zero-copy", 4, start=777), K("istft_frame_f32", 1000, 1, "staged", start=300_001),
           K("stft_magnitudes_f32", 1024, 37, "zero-copy", 4, hop=256), K("stft_magnitudes_f32", 1024, 2051, "staged", hop=256)]
    for call, a in (("fftnd_c32", 8), ("fftnd_c64", 16)):
        cs += [K(call, 24, 128, "zero-copy", a), K(call, 512, 512, "staged", inverse=1), K(call, 7, 5, "zero-copy", a, depth=6)]
    # the chunked upload / kernel / download pipeline: at least 128 MiB in + out, a batch that does not divide by eight
    cs += [K("fft_c32", 4096, 4099, "pipeline"), K("rfft_f32", 2048, 8203, "pipeline", window=1)]
    return cs


DEV_CASES = _dev_cases()
HOST_CASES = _host_cases()

DEV_DRIVERS = {"fft_c32_dev": drv_fft_inplace, "fft_c64_dev": drv_fft_inplace, "fft_c32_dev_oop": drv_fft_oop, "fft_c64_dev_oop": drv_fft_oop,
               "fft_radix4_c32_dev": drv_radix4, "fft_radix4_c64_dev": drv_radix4, "ifft_radix4_c32_dev": drv_radix4, "ifft_radix4_c64_dev": drv_radix4,
               "rfft_f32_dev": drv_rfft, "rfft_f64_dev": drv_rfft, "irfft_f32_dev": drv_irfft, "irfft_f64_dev": drv_irfft,
               "dct2_f32_dev": drv_rowwise, "hilbert_f32_dev": drv_rowwise, "cepstrum_f32_dev": drv_rowwise,
               "dct_direct_f32_dev": drv_direct, "dst_direct_f32_dev": drv_direct,
               "dwt_f32_dev": drv_dwt, "idwt_f32_dev": drv_idwt, "dwt_multi_f32_dev": drv_dwt_multi, "idwt_multi_f32_dev": drv_idwt_multi,
               "stft_f32_dev": drv_stft_dev, "istft_f32_dev": drv_istft, "stft_magnitudes_f32_dev": drv_magnitudes,
               "fftnd_c32_dev": drv_fftnd, "fftnd_c64_dev": drv_fftnd}
HOST_DRIVERS = {"fft_c32": drv_fft_inplace, "fft_c64": drv_fft_inplace, "fft_c32_strided": drv_strided, "fft_c64_strided": drv_strided,
                "rfft_f32": drv_rfft, "rfft_f64": drv_rfft, "irfft_f32": drv_irfft, "irfft_f64": drv_irfft,
                "dct2_f32": drv_rowwise, "hilbert_f32": drv_rowwise, "cepstrum_f32": drv_rowwise, "dct_direct_f32": drv_direct, "dst_direct_f32": drv_direct,
                "dwt_f32": drv_dwt, "idwt_f32": drv_idwt, "dwt_multi_f32": drv_dwt_multi, "idwt_multi_f32": drv_idwt_multi,
                "stft_f32": drv_stft_host, "stft_parallel_f32": drv_stft_host, "stft_frame_f32": drv_stft_frame,
                "istft_f32": drv_istft, "istft_parallel_f32": drv_istft_parallel, "istft_frame_f32": drv_istft_frame,
                "stft_magnitudes_f32": drv_magnitudes, "fftnd_c32": drv_fftnd, "fftnd_c64": drv_fftnd}


# ---- the tests --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env(oracle):
    """One f32 and one f64 context for every case of the module (route switches are put back by the drivers)."""
    import kofft_amd

    E = SimpleNamespace(f32=kofft_amd.HipFftImpl(np.float32), f64=kofft_amd.HipFftImpl(np.float64), oracle=oracle)
    yield E
    E.f32.close()
    E.f64.close()


@pytest.mark.parametrize("case", DEV_CASES, ids=case_id)
def test_device_pointer_footprint(env, case):
    DEV_DRIVERS[case.call](env, case, True)


@pytest.mark.parametrize("case", HOST_CASES, ids=case_id)
def test_host_pointer_footprint(env, oracle, monkeypatch, case):
    if case.route != "pipeline":
        HOST_DRIVERS[case.call](env, case, False)
        return
    import kofft_amd

    monkeypatch.setenv("KOFFT_HIP_HOST_PIPELINE", "1")  # read when a context is created
    f = kofft_amd.HipFftImpl(np.float32)
    try:
        HOST_DRIVERS[case.call](SimpleNamespace(f32=f, f64=None, oracle=oracle), case, False)
    finally:
        f.close()


def _one_row_after(err, region, row_bytes):
    hits = [h for h in err.findings if h["region"] == region]
    assert len(err.findings) == 1 and len(hits) == 1, str(err)
    h = hits[0]
    # (a byte of the row may equal the pattern's byte at its place: the run may start or end a few bytes inside the row)
    assert h["side"] == "after" and 0 <= h["first"] < 8 and row_bytes - 8 < h["span"] <= row_bytes and h["last"] < row_bytes, str(err)
    assert "rows" in str(err)


def test_sensitivity_fft_oop_one_row_too_many(env):
    """The module can fail: batch rows written into an output the arena holds batch - 1 rows for -- the last row lands in the band
    (inside the arena's own allocation) and verify() reports one row directly after the region."""
    f, n, batch = env.f32, 1024, 5
    arena = Arena("cuda", "sensitivity fft_c32_dev_oop")
    x = _rc(np.random.default_rng(77), (batch, n))
    i = arena.input(x, row_bytes=8 * n, name="in")
    out = arena.output(8 * n * (batch - 1), row_bytes=8 * n, name="out")
    for _ in range(2):
        f._check(f._lib.kofft_hip_fft_c32_dev_oop(f._ctx, _p(i), _p(out), n, batch, 0))
    f.synchronize()
    with pytest.raises(RedzoneError) as e:
        arena.verify()
    _one_row_after(e.value, "out", 8 * n)
    assert_rows_equal(arena.read(out, np.complex64, (batch - 1, n)), env.oracle.fft_mt(x)[:batch - 1], "sensitivity: the rows inside")


def test_sensitivity_dwt_multi_one_row_too_many(env):
    c = K("dwt_multi_f32_dev", 1000, 9, "level", wavelet="db2", levels=3)
    with pytest.raises(RedzoneError) as e:
        drv_dwt_multi(env, c, True, short_rows=1)
    _one_row_after(e.value, "approx", 4 * wo.multi_lengths(1000, 3)[-1])


def test_case_sizes():
    """Every case but the streaming and pipeline ones holds at most 2^22 points in + out (row-wise and complex families)."""
    for c in DEV_CASES + HOST_CASES:
        if c.route in ("stream", "pipeline") or not re.match(r"(i?fft|i?rfft|dct2|hilbert|cepstrum|fftnd)", c.call):
            continue
        pts = c.n * c.batch * int(dict(c.opt).get("depth", 1))
        oop = not (c.call in ("fft_c32_dev", "fft_c64_dev", "fft_c32", "fft_c64") or "fftnd" in c.call or "strided" in c.call or dict(c.opt).get("same"))
        assert pts * (2 if oop else 1) <= MAX_POINTS, case_id(c)
