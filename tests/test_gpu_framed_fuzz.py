"""Seeded frame-geometry fuzz over the families that cut rows of samples into frames: stft_rows, stft_magnitudes_rows,
stft_onesided, the one-sided and the parallel inverse, stft_mel, stft_mfcc, stft_picture, welch, csd and the overlap-save convolve, on
TWO contexts shared by every case of the module -- the default one and one created under KOFFT_HIP_SCRATCH_CHUNK_MB=1 -- whose route
switches change from case to case, so that table cache, grow-only scratch and routes are whatever the calls before left behind.

tests/framed_cases.py draws the cases (one geometry per case, every family called on it in an order of the case's own rng) and
tests/framed_expected.py derives every expected value from one pass of the CPU oracle.  Every row of every output is compared bit
for bit (NaN-safe); every call runs twice on buffers inside a guard-band arena (tests/redzone.py; the host forms on a host arena):
the same bytes twice, inputs and NaN gaps unchanged, nothing written outside an output, max_out exactly `rows` floats.  A call the
header refuses returns its code and leaves the prefilled output alone; the next family is checked as usual.  One case per seed
releases the scratch between two families, another runs one family on a side stream.  The one-sided frames of finite cases are held
to rfft in float64 within the bound of tests/test_framed_cases_cpu.py.  A failure names seed, case, family, route, form and the
geometry."""
import numpy as np
import pytest

import framed_cases as fc
import framed_expected as fe
from redzone import Arena
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32
KNOB = "KOFFT_HIP_SCRATCH_CHUNK_MB"
ISTFT_MAX_OUT = 1 << 21


def _defaults(f):
    f.set_welch_fused(1)
    f.set_frontend_fused(1)
    f.set_mfcc_fused(1)
    f.set_convolve_fused(True)
    f._check(f._lib.kofft_hip_set_spectrogram_transpose(f._ctx, 1))


@pytest.fixture(scope="module")
def contexts():
    """The two contexts of the module; the knob is read when a context is created and is put back right after."""
    import kofft_amd

    default = kofft_amd.HipFftImpl(F)
    mp = pytest.MonkeyPatch()
    mp.setenv(KNOB, "1")
    try:
        chunk1 = kofft_amd.HipFftImpl(F)
    finally:
        mp.undo()
    both = {"default": default, "chunk1": chunk1}
    yield both
    for f in both.values():
        _defaults(f)
        f.close()


class Call:
    """One family call on buffers of a guard-band arena: regions first, then run(): twice, the same bytes, the bands intact."""

    def __init__(self, f, form, what):
        self.f, self.form, self.what = f, form, what
        self.host = form == "host"
        self.arena = Arena("host" if self.host else "cuda", what)
        self.off4 = 4 if form == "dev_off" else 0   # every f32 pointer 4 bytes off a 16-byte boundary
        self.off8 = 8 if form == "dev_off" else 0   # complex outputs stay 8-byte aligned
        self.off1 = 1 if form == "dev_off" else 0   # pictures need no alignment
        self.outs = []

    def fn(self, stem):
        return getattr(self.f._lib, ("kofft_hip_" if self.host else "kofft_hip_dev_") + stem)

    def input(self, a, name, row_bytes=None, off=None):
        return self.arena.input(a, self.off4 if off is None else off, row_bytes, name)

    def output(self, nbytes, name, off, prefill=None, row_bytes=None):
        r = self.arena.output(nbytes, off, prefill, row_bytes, name)
        self.outs.append(r)
        return r

    def _read(self):
        self.f.synchronize()
        return [self.arena.read(r, np.uint8, (r.nbytes,)) for r in self.outs]

    def run(self, invoke, refused=None, stream=None):
        """invoke() -> the return code.  Returns the outputs' bytes (None for a refused call)."""
        for r in self.arena.regions:
            r.addr  # (lays the arena out before the first call)
        if stream is not None:
            self.f.set_stream(stream.cuda_stream)
        try:
            rc = invoke()
            first = self._read()
            if refused is not None:
                assert rc == refused, f"{self.what}: returned {rc}, the header says {refused}"
                for r, b in zip(self.outs, first):
                    assert b.tobytes() == self.arena._host(r.start, r.start + r.nbytes, pristine=True).tobytes(), \
                        f"{self.what}: a refused call wrote to '{r.name}'"
                self.arena.verify()
                return None
            assert rc == 0, f"{self.what}: returned {rc}"
            for r in self.outs:
                self.arena.restore(r)
            rc = invoke()
            assert rc == 0, f"{self.what}: the second run returned {rc}"
            second = self._read()
        finally:
            if stream is not None:
                self.f.synchronize()
                self.f.set_stream(0)
        for r, a, b in zip(self.outs, first, second):
            assert a.tobytes() == b.tobytes(), f"{self.what}: two runs of the same call differ in '{r.name}'"
        self.arena.verify()
        return first


def _frames2d(a, width):
    return np.ascontiguousarray(a).reshape(-1, width) if width else np.ascontiguousarray(a).reshape(a.shape[0], -1)


def _route(case, fam):
    if fam in ("welch", "csd"):
        return fc.welch_route(case)
    if fam == "mel":
        return fc.frontend_route(case)
    if fam == "mfcc":
        return f"{fc.frontend_route(case)}/{fc.mfcc_route(case)}"
    return "kernels" if fc.kernels_cover(case.win_len) else "bluestein"


def _family(f, case, fam, inp, exp, stream):
    """Run one family of a framed case and compare it with its expected value; returns the one-sided frames where fam is that family."""
    w, hop, rows, length, stride = case.win_len, case.hop, case.rows, case.len, case.row_stride
    frames, form = case.frames[fam], case.forms[fam]
    K, half = w // 2 + 1, w // 2
    what = (f"{case.describe()} family={fam} route={_route(case, fam)} form={form} frames={frames} modes=(welch {case.welch_fused}, frontend "
            f"{case.frontend_fused}, mfcc {case.mfcc_fused}, transpose {case.transpose})")
    want = exp[fam]
    refused = want.code if isinstance(want, fe.Refused) else None
    c = Call(f, form, what)
    sig = c.input(fc.strided(case, inp["x"]), "signal", 4 * stride)
    hann_given = fam in ("stft", "onesided")  # these two take no null window
    win = c.input(exp["window"], "window") if (inp["window"] is not None or hann_given) else None
    wp = lambda: win.addr if win is not None else None
    ctx = f._ctx
    if fam == "stft":
        out = c.output(rows * frames * w * 8, "frames", c.off8, row_bytes=8 * w)
        got = c.run(lambda: c.fn("stft_rows_f32")(ctx, sig.addr, rows, length, stride, wp(), w, hop, out.addr, frames), refused, stream)
        if got is not None:
            assert_rows_equal(got[0].view(np.complex64).reshape(-1, w), _frames2d(want, w), what, nan_safe=True)
    elif fam == "onesided":
        out = c.output(rows * frames * K * 8, "one-sided frames", c.off8, row_bytes=8 * K)
        got = c.run(lambda: c.fn("stft_onesided_f32")(ctx, sig.addr, rows, length, stride, wp(), w, hop, out.addr, frames), refused, stream)
        if got is not None:
            half_got = got[0].view(np.complex64).reshape(rows, frames, K)
            assert_rows_equal(half_got.reshape(-1, K), _frames2d(want, K), what, nan_safe=True)
            return half_got
    elif fam == "mags":
        out = c.output(rows * frames * half * 4, "magnitudes", c.off4, row_bytes=4 * half)
        mx = c.output(rows * 4, "max_mag", c.off4)
        got = c.run(lambda: c.fn("stft_magnitudes_rows_f32")(ctx, sig.addr, rows, length, stride, w, hop, out.addr, frames, mx.addr), refused, stream)
        if got is not None:
            if half:
                assert_rows_equal(got[0].view(F).reshape(rows * frames, half), _frames2d(want[0], half), what, nan_safe=True)
            assert_rows_equal(got[1].view(F), want[1], what + " max_mag", nan_safe=True)
    elif fam in ("mel", "mfcc"):
        cols = case.num_mel if fam == "mel" else case.num_coeffs
        out = c.output(rows * frames * cols * 4, "energies" if fam == "mel" else "coefficients", c.off4, row_bytes=4 * cols)
        bins = inp["bins"]
        if fam == "mel":
            call = lambda: c.fn("stft_mel_f32")(ctx, sig.addr, rows, length, stride, wp(), w, hop, frames, bins.ctypes.data, case.num_mel, out.addr)
        else:
            call = lambda: c.fn("stft_mfcc_f32")(ctx, sig.addr, rows, length, stride, wp(), w, hop, frames, bins.ctypes.data, case.num_mel,
                                                 case.num_coeffs, out.addr)
        got = c.run(call, refused, stream)
        if got is not None:
            assert_rows_equal(got[0].view(F).reshape(rows * frames, cols), _frames2d(want, cols), what, nan_safe=True)
    elif fam == "picture":
        p = case.picture
        px = p["channels"] * p["depth"] // 8
        what += f" picture={p}"
        c.what = c.arena.what = what
        out = c.output(rows * frames * half * px, "pictures", c.off1, row_bytes=(frames if p["layout"] == 1 else half) * px)
        mx = c.output(rows * 4, "max_out", c.off4)
        max_in = c.input(inp["max_in"], "max_in") if p["max_mode"] == 2 else None
        table = inp["table"]
        tp = table.ctypes.data if table is not None else None
        got = c.run(lambda: c.fn("stft_picture_f32")(ctx, sig.addr, rows, length, stride, wp(), w, hop, frames, p["max_mode"],
                                                     max_in.addr if max_in is not None else None, mx.addr, p["mode"], p["level"], p["cmap"],
                                                     p["depth"], p["channels"], p["scale"], p["layout"], tp, out.addr), refused, stream)
        if got is not None:
            pics, want_max = want
            if half:
                width = pics.shape[-2] * pics.shape[-1]
                assert_rows_equal(got[0].view(pics.dtype).reshape(-1, width), pics.reshape(-1, width), what)
            assert_rows_equal(got[1].view(F), want_max, what + " max_out", nan_safe=True)
    elif fam in ("welch", "csd"):
        vals = K * (2 if fam == "csd" else 1)
        out = c.output(rows * vals * 4, "spectra", c.off8 if fam == "csd" else c.off4, row_bytes=4 * vals)
        flags = 1 if case.welch_double else 0
        if fam == "welch":
            call = lambda: c.fn("welch_f32")(ctx, sig.addr, rows, length, stride, wp(), w, hop, frames, case.welch_scale, flags, out.addr)
        else:
            other = c.input(fc.strided(case, inp["y"]), "y", 4 * stride)
            call = lambda: c.fn("csd_f32")(ctx, sig.addr, other.addr, rows, length, stride, wp(), w, hop, frames, case.welch_scale, flags, out.addr)
        got = c.run(call, refused, stream)
        if got is not None:
            assert_rows_equal(got[0].view(want.dtype).reshape(rows, K), want, what, nan_safe=True)
    return None


def _istft(f, case, inp, exp, half_got):
    """istft_onesided of the one-sided frames the device returned and istft_parallel_rows of their completion, both accumulating into
    the same prefilled output: the same bits."""
    w, hop, rows = case.win_len, case.hop, case.rows
    frames, form = half_got.shape[1], case.forms["istft"]
    K = w // 2 + 1
    out_len = min((frames - 1) * hop + w, ISTFT_MAX_OUT // rows)
    if case.len and case.data_seed % 2:
        out_len = min(out_len, case.len)
    full = fe.onesided_ref.complete(half_got, w)
    prefill = np.resize(inp["prefill"], rows * out_len).astype(F)
    res = []
    for name, stem, data, width in (("istft_onesided", "istft_onesided_f32", half_got, K), ("istft_parallel_rows", "istft_parallel_rows_f32", full, w)):
        what = f"{case.describe()} family={name} route={'kernels' if fc.kernels_cover(w) else 'bluestein'} form={form} frames={frames} out_len={out_len}"
        c = Call(f, form, what)
        src = c.input(data, "frames", 8 * width, off=c.off8)
        win = c.input(exp["window"], "window")
        out = c.output(rows * out_len * 4, "output", c.off4, prefill=prefill, row_bytes=4 * out_len)
        got = c.run(lambda: c.fn(stem)(f._ctx, src.addr, rows, frames, win.addr, w, hop, out.addr, out_len))
        res.append(got[0].view(F).reshape(rows, out_len))
    assert_rows_equal(res[0], res[1], f"{case.describe()} family=istft_onesided against istft_parallel_rows form={form} frames={frames} out_len={out_len}",
                      nan_safe=True)


def _framed_case(f, oracle, case):
    import torch

    f.set_welch_fused(case.welch_fused)
    f.set_frontend_fused(case.frontend_fused)
    f.set_mfcc_fused(case.mfcc_fused)
    f._check(f._lib.kofft_hip_set_spectrogram_transpose(f._ctx, case.transpose))
    inp = fc.inputs(case)
    with np.errstate(all="ignore"):
        exp = fe.expected(oracle, case, inp)
        half_got = None
        for k, fam in enumerate(fc.family_order(case)):
            if k == case.release_after:
                f.release_scratch()
            stream = torch.cuda.Stream() if fam == fc.stream_family(case) else None  # (a host form stages through that stream)
            got = _family(f, case, fam, inp, exp, stream)
            if got is not None:
                half_got = got
        if half_got is not None:
            _istft(f, case, inp, exp, half_got)
            bound = fe.float64_bound(case.win_len)
            if not case.specials and bound is not None:
                for err in fe.float64_errors(case, inp, exp["window"], half_got):
                    assert err <= bound, f"{case.describe()} family=onesided: float64 rel err {err:.3g} > {bound:.3g}"


def _convolve_case(f, c):
    f.set_convolve_fused(bool(c.fused))
    inp = fc.conv_inputs(c)
    want = fe.conv_expected(c, inp)
    what = c.describe()
    call = Call(f, c.form, what)
    x = call.input(inp["x"], "x", 4 * c.nx)
    h = call.input(inp["h"], "h", 4 * c.nh)
    out = call.output(c.rows * c.out_len * 4, "out", call.off4, row_bytes=4 * c.out_len)
    filters = c.rows if inp["h"].ndim == 2 else 1
    got = call.run(lambda: call.fn("convolve_f32")(f._ctx, x.addr, c.rows, c.nx, h.addr, filters, c.nh, c.block, 1 if c.correlate else 0, out.addr,
                                                   c.out_first, c.out_len))
    got = got[0].view(F).reshape(c.rows, c.out_len)
    assert_rows_equal(got, want, what, nan_safe=True)
    err = fe.conv_float64_error(c, inp, got.astype(np.float64), c.out_first)
    if err is not None:
        assert err <= fe.conv_float64_bound(c.block), f"{what}: float64 rel err {err:.3g}"


@pytest.mark.parametrize("seed", range(fc.SEEDS))
def test_fuzz_framed(contexts, oracle, seed):
    try:
        for case in fc.cases(seed):
            f = contexts[case.ctx]
            if case.kind == "convolve":
                _convolve_case(f, case)
            else:
                _framed_case(f, oracle, case)
    finally:
        for f in contexts.values():
            _defaults(f)
