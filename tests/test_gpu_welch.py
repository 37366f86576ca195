"""Welch power spectra and cross spectra of rows on the device, bit for bit against tests/welch_oracle.py.  Power-of-two
windows of 64 .. 4096 samples have welch_fused_kernel<6 .. 12> (one instance each for the power and the cross spectrum, then
welch_total_kernel where a row has more than one group of 32 frames); every other window -- and every window in a context with
set_welch_fused(0) -- runs the one-sided STFT into the scratch, welch_partial_kernel and welch_total_kernel.  Every case runs on a
default context, a composed one (mode 0) and a fused one (mode 2), and all three must give the oracle's bytes."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import welch_oracle as wo
from conftest import bits_equal, seeded
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = Path(__file__).resolve().parent.parent
VARIANTS = [(1.0, False), (0.3, True), (0.3, False), (1.0, True)]  # (scale, KOFFT_HIP_PSD_DOUBLE)


@pytest.fixture(scope="module")
def routes(fft32):
    """(name, context): the default rule, every call composed, the fused kernel wherever it exists."""
    import kofft_amd

    composed, fused = kofft_amd.HipFftImpl(F), kofft_amd.HipFftImpl(F)
    composed.set_welch_fused(0)
    fused.set_welch_fused(2)
    yield [("default", fft32), ("composed", composed), ("fused", fused)]
    composed.close()
    fused.close()


def _host(f, x, y, win_len, hop, frames, window, scale, double):
    if y is None:
        return f.welch_rows(x, win_len, hop, frames, window, scale, double)
    return f.csd_rows(x, y, win_len, hop, frames, window, scale, double)


def _dev(f, x, y, win_len, hop, frames, window, scale, double, off=0, stride=None):
    """The device entries on torch buffers: off floats into every allocation, rows `stride` apart with NaN in the gaps, the output
    prefilled with NaN."""
    import torch

    rows, length = x.shape
    stride = length if stride is None else stride
    K = win_len // 2 + 1
    vals = K * (1 if y is None else 2)

    def up(a):
        d = torch.full((off + rows * stride,), float("nan"), dtype=torch.float32, device="cuda")
        d[off:].view(rows, stride)[:, :length] = torch.from_numpy(a).cuda()
        return d

    dx = up(x)
    dy = None if y is None else up(y)
    dw = None
    if window is not None:
        dw = torch.zeros(off + win_len, dtype=torch.float32, device="cuda")
        dw[off:] = torch.from_numpy(window).cuda()
    out = torch.full((off + rows * vals,), float("nan"), dtype=torch.float32, device="cuda")
    wp = 0 if dw is None else dw.data_ptr() + 4 * off
    if y is None:
        f.welch_rows_dev(dx.data_ptr() + 4 * off, rows, length, stride, wp, win_len, hop, frames, out.data_ptr() + 4 * off, scale, double)
    else:
        f.csd_rows_dev(dx.data_ptr() + 4 * off, dy.data_ptr() + 4 * off, rows, length, stride, wp, win_len, hop, frames,
                       out.data_ptr() + 4 * off, scale, double)
    f.synchronize()
    got = out[off:].cpu().numpy().reshape(rows, vals)
    return got if y is None else np.ascontiguousarray(got).view(np.complex64)


def _all_routes(routes, x, y, win_len, hop, frames, window, want_window, what, variants=VARIANTS, nan_safe=False, run=_host, **kw):
    """Every variant on every route against the oracle (one pass of the oracle over the frames, finished per variant)."""
    totals = wo.welch_totals(x, want_window, hop, frames, y)
    for scale, double in variants:
        want = wo.finish(totals, win_len, scale, double)
        for name, f in routes:
            got = run(f, x, y, win_len, hop, frames, window, scale, double, **kw)
            assert_rows_equal(got, want, f"{what} scale={scale} double={double}: {name} route", nan_safe=nan_safe)


@pytest.mark.parametrize("frames", wo.GRID_FRAMES)
@pytest.mark.parametrize("win_len", wo.GRID_WINS)
def test_group_edge_grid(routes, oracle, win_len, frames):
    """frames 1, 31, 32, 33, 65 (one group short, full, one and two groups and a bit), rows 1 and 3, hops win_len / 4, win_len, win_len
    + 3 (and 1 at 64), both flags, two scales; the last frame of every row runs past its end.  window None is hann(win_len)."""
    hann = oracle.hann(win_len)
    for rows in wo.GRID_ROWS:
        for hop in wo.grid_hops(win_len):
            x = wo.grid_input(win_len, hop, frames, rows)
            explicit = hop == win_len  # a caller's window on one hop of three
            _all_routes(routes, x, None, win_len, hop, frames, hann if explicit else None, hann, f"win_len={win_len} frames={frames} rows={rows} hop={hop}")
    x = wo.grid_input(win_len, win_len // 4, frames, 3)
    _all_routes(routes, x, None, win_len, win_len // 4, frames, None, hann, f"win_len={win_len} frames={frames} dev", variants=VARIANTS[:2], run=_dev)


@pytest.mark.parametrize("win_len,hop,frames,window", [(400, 160, 40, "hamming"), (6, 2, 70, None), (5, 3, 33, None), (8192, 2048, 34, None),
                                                       (2048, 512, 40, None)])
def test_odd_and_unusual_lengths(routes, oracle, win_len, hop, frames, window):
    """A Bluestein length with Hamming, a tiny even length, an odd one (no Nyquist bin: every bin but 0 is doubled), a length past the
    fused kernel, the fused length whose default is the composed route."""
    from kofft_amd import window as W

    win = np.ascontiguousarray(W.hamming(win_len), F) if window == "hamming" else None
    x = wo.grid_input(win_len, hop, frames, 3)
    _all_routes(routes, x, None, win_len, hop, frames, win, oracle.hann(win_len) if win is None else win, f"win_len={win_len} hop={hop}")
    _all_routes(routes, x, None, win_len, hop, frames, win, oracle.hann(win_len) if win is None else win, f"win_len={win_len} hop={hop} dev",
                variants=VARIANTS[:2], run=_dev)


@pytest.mark.parametrize("win_len", [64, 400, 1024])
def test_rows_and_tails(routes, oracle, win_len):
    """Rows shorter than the window (every frame partial, most of them empty), and two frames more than the signal fills."""
    hann = oracle.hann(win_len)
    hop = win_len // 4
    x = seeded(26100 + win_len).standard_normal((3, win_len - 7)).astype(F)
    for frames in (1, 3, 35):
        _all_routes(routes, x, None, win_len, hop, frames, None, hann, f"short rows win_len={win_len} frames={frames}", variants=VARIANTS[:2])
    x = seeded(26101 + win_len).standard_normal((3, 40 * hop + 5)).astype(F)
    frames = -(-x.shape[1] // hop) + 2
    _all_routes(routes, x, None, win_len, hop, frames, None, hann, f"frames past the signal win_len={win_len}", variants=VARIANTS[:2])
    _all_routes(routes, x, x[::-1].copy(), win_len, hop, frames, None, hann, f"csd frames past the signal win_len={win_len}", variants=VARIANTS[:2])


@pytest.mark.parametrize("win_len", [64, 400, 1024])
def test_special_values(routes, oracle, win_len):
    """N(0, 1) with +-0, subnormals, one Inf and one NaN: NaNs come out exactly where the oracle has them."""
    hann = oracle.hann(win_len)
    hop, frames = win_len // 4, 70
    x = wo.grid_input(win_len, hop, frames, 3)
    x[0, :6] = [0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -0.0]
    x[1] = -0.0
    x[1, 5 * hop:5 * hop + 3] = [1e-40, -1e-41, 3e-39]
    _all_routes(routes, x, None, win_len, hop, frames, None, hann, f"zeros and subnormals win_len={win_len}", variants=VARIANTS[:2], nan_safe=True)
    x[0, 40 * hop + 1] = np.nan
    x[2, 3 * hop + 2] = np.inf
    want = wo.welch_ref(x, hann, hop, frames)
    assert np.isnan(want[0]).all() and not np.isnan(want[1]).any()
    _all_routes(routes, x, None, win_len, hop, frames, None, hann, f"NaN and Inf win_len={win_len}", variants=VARIANTS[:2], nan_safe=True)
    y = wo.grid_input(win_len, hop, frames, 3, 1)
    _all_routes(routes, x, y, win_len, hop, frames, None, hann, f"csd NaN and Inf win_len={win_len}", variants=VARIANTS[:2], nan_safe=True)


@pytest.mark.parametrize("frames", wo.GRID_FRAMES)
@pytest.mark.parametrize("win_len", [64, 400, 1024])
def test_csd_grid(routes, oracle, win_len, frames):
    hann = oracle.hann(win_len)
    for rows in wo.GRID_ROWS:
        for hop in wo.grid_hops(win_len):
            x = wo.grid_input(win_len, hop, frames, rows)
            y = wo.grid_input(win_len, hop, frames, rows, 1)
            _all_routes(routes, x, y, win_len, hop, frames, None, hann, f"csd win_len={win_len} frames={frames} rows={rows} hop={hop}")
    _all_routes(routes, x, y, win_len, hop, frames, hann, hann, f"csd win_len={win_len} frames={frames} dev", variants=VARIANTS[:2], run=_dev)


@pytest.mark.parametrize("win_len", [64, 400, 1024])
def test_csd_identities(routes, win_len):
    """csd(x, x): the real part is welch(x) bit for bit and the imaginary part exactly zero; csd(y, x) == conj(csd(x, y)) by value."""
    hop, frames = win_len // 4, 65
    x = wo.grid_input(win_len, hop, frames, 3)
    y = wo.grid_input(win_len, hop, frames, 3, 1)
    for name, f in routes:
        for scale, double in VARIANTS[:2]:
            pxx = f.welch_rows(x, win_len, hop, frames, None, scale, double)
            cxx = f.csd_rows(x, x, win_len, hop, frames, None, scale, double)
            assert_rows_equal(np.ascontiguousarray(cxx.real), pxx, f"csd(x, x).real win_len={win_len} {name}")
            assert not cxx.imag.any(), f"csd(x, x).imag win_len={win_len} {name}"
            cxy = f.csd_rows(x, y, win_len, hop, frames, None, scale, double)
            cyx = f.csd_rows(y, x, win_len, hop, frames, None, scale, double)
            assert np.array_equal(cyx, np.conj(cxy)), f"csd(y, x) win_len={win_len} {name}"


@pytest.mark.parametrize("win_len", [256, 400])
def test_device_forms(routes, oracle, win_len):
    """4-byte aligned views, row_stride > len with NaN in the gaps, NaN-prefilled outputs, another stream, release_scratch between
    calls; the overlap refusals, then one valid call."""
    import torch

    import kofft_amd

    hann = oracle.hann(win_len)
    hop, frames, rows = win_len // 2, 45, 3
    x = wo.grid_input(win_len, hop, frames, rows)
    y = wo.grid_input(win_len, hop, frames, rows, 1)
    for off, stride in ((1, None), (0, x.shape[1] + 5), (3, x.shape[1] + 1)):
        for other in (None, y):
            _all_routes(routes, x, other, win_len, hop, frames, hann, hann, f"dev off={off} stride={stride} csd={other is not None}",
                        variants=VARIANTS[:2], run=_dev, off=off, stride=stride)
    want = wo.welch_ref(x, hann, hop, frames, 0.3, True)
    stream = torch.cuda.Stream()
    for name, f in routes:
        f.set_stream(stream.cuda_stream)
        try:
            with torch.cuda.stream(stream):
                assert_rows_equal(_dev(f, x, None, win_len, hop, frames, None, 0.3, True), want, f"another stream {name}")
        finally:
            f.set_stream(0)
        f.release_scratch()
        assert_rows_equal(_dev(f, x, None, win_len, hop, frames, None, 0.3, True), want, f"after release_scratch {name}")
        f.release_scratch()
        assert_rows_equal(_host(f, x, None, win_len, hop, frames, None, 0.3, True), want, f"host after release_scratch {name}")
    # the refusals: the output on the signal, on the second signal, on the window
    K = win_len // 2 + 1
    f = routes[0][1]
    buf = torch.zeros(rows * x.shape[1] + 2 * rows * K + win_len, dtype=torch.float32, device="cuda")
    sig, win = buf.data_ptr(), buf.data_ptr() + 4 * rows * x.shape[1]
    free = win + 4 * win_len
    E = kofft_amd.FftError
    for call in (lambda: f.welch_rows_dev(sig, rows, x.shape[1], x.shape[1], 0, win_len, hop, frames, sig + 4 * (x.shape[1] - 1)),
                 lambda: f.welch_rows_dev(sig, rows, x.shape[1], x.shape[1], win, win_len, hop, frames, win + 4 * (win_len - 1)),
                 lambda: f.welch_rows_dev(sig, rows, x.shape[1], x.shape[1], win, win_len, hop, frames, win - 4 * rows * K + 4),
                 lambda: f.csd_rows_dev(free, sig, rows, x.shape[1], x.shape[1], 0, win_len, hop, frames, sig + 8),
                 lambda: f.csd_rows_dev(sig, free, rows, x.shape[1], x.shape[1], 0, win_len, hop, frames, sig)):
        with pytest.raises(E) as e:
            call()
        assert e.value.code == 6
    assert_rows_equal(_dev(f, x, None, win_len, hop, frames, None, 0.3, True), want, "a valid call after the refusals")


def test_second_context(routes, oracle):
    """Two contexts in turn on the same inputs: each keeps its own scratch and tables."""
    import kofft_amd

    win_len, hop, frames = 512, 128, 70
    hann = oracle.hann(win_len)
    x = wo.grid_input(win_len, hop, frames, 3)
    want = wo.welch_ref(x, hann, hop, frames, 0.3, True)
    other = kofft_amd.HipFftImpl(F)
    try:
        for _ in range(2):
            for f in (routes[0][1], other):
                assert_rows_equal(f.welch_rows(x, win_len, hop, frames, None, 0.3, True), want, "second context")
    finally:
        other.close()


def test_module_functions(routes, oracle):
    """kofft_amd.psd.welch / csd: whole segments only, the library's scale, 1-D and 2-D inputs, against the oracle and (loosely) scipy."""
    from scipy import signal

    from kofft_amd import psd

    win_len, hop = 256, 128
    x = seeded(26300).standard_normal((3, 5000)).astype(F)
    y = seeded(26301).standard_normal((3, 5000)).astype(F)
    frames = psd.segments(5000, win_len, hop)
    assert frames == 38
    hann = oracle.hann(win_len)
    for scaling in ("density", "spectrum"):
        s = psd.scale(None, win_len, 8000.0, frames, scaling)
        for name, f in routes:
            freqs, pxx = psd.welch(x, win_len, fs=8000.0, scaling=scaling, fft=f)
            assert freqs.shape == (129,) and freqs[1] == 8000.0 / 256
            assert_rows_equal(pxx, wo.welch_ref(x, hann, hop, frames, s, True), f"psd.welch {scaling} {name}")
            _, pxy = psd.csd(x, y, win_len, fs=8000.0, scaling=scaling, onesided_double=False, fft=f)
            assert_rows_equal(pxy, wo.welch_ref(x, hann, hop, frames, s, False, y=y), f"psd.csd {scaling} {name}")
    _, p1 = psd.welch(x[0], win_len, fs=8000.0, fft=routes[0][1])
    assert p1.shape == (129,) and bits_equal(p1, psd.welch(x, win_len, fs=8000.0, fft=routes[0][1])[1][0])
    _, want64 = signal.welch(x[0].astype(np.float64), fs=8000.0, window=hann.astype(np.float64), nperseg=win_len, noverlap=win_len - hop,
                             detrend=False)
    assert np.max(np.abs(p1 - want64)) <= 4 * 9.893e-7 * np.max(want64)  # tests/test_welch_cpu.py's bound at 256


@pytest.mark.parametrize("csd,rows,frames,want", [(False, 7, 1500, (3896, 3892, (604, 3000, 288))), (True, 8, 600, (1928, 1928, (472, 1200, 256)))],
                         ids=["welch-7x1500", "csd-8x600"])
def test_a_chunk_with_the_tail_of_a_row_whole_rows_and_the_head_of_a_row(monkeypatch, fft32, csd, rows, frames, want):
    """KOFFT_HIP_SCRATCH_CHUNK_MB=1, win_len 64 on the composed route (set_welch_fused(0)): the one-sided frames come from the STFT
    kernels per rectangle of the chunk, and the second chunk holds the tail of a row, two whole rows and the head of a row (its ends
    are group seams).  Against the oracle and against the same call on a default context, bit for bit."""
    import framed_cases as fc
    import kofft_amd
    from oracle import pyoracle
    from test_gpu_scratch_seams import chunk_kinds

    win_len, hop, total = 64, 4, rows * frames
    cap = fc.welch_composed_cap(win_len, csd, 1 << 20, total)
    t0 = fc.welch_chunk_end(0, cap, frames, total)
    nt = fc.welch_chunk_end(t0, cap, frames, total) - t0
    assert (t0, nt, chunk_kinds(t0, nt, frames)) == want and all(want[2])
    length = (frames - 1) * hop + win_len - 3
    assert fc.welch_frames_walked(length, hop, frames) == frames
    rng = seeded(26500 + rows)
    x = rng.standard_normal((rows, length)).astype(F)
    y = rng.standard_normal((rows, length)).astype(F) if csd else None
    ref = wo.welch_ref(x, pyoracle.hann(win_len), hop, frames, 0.3, True, y=y)
    monkeypatch.setenv("KOFFT_HIP_SCRATCH_CHUNK_MB", "1")
    f = kofft_amd.HipFftImpl(F)
    try:
        f.set_welch_fused(0)
        got = _host(f, x, y, win_len, hop, frames, None, 0.3, True)
        assert_rows_equal(got, ref, f"three kinds of rectangle in one chunk, csd={csd}")
        assert bits_equal(got, _host(fft32, x, y, win_len, hop, frames, None, 0.3, True)), "differs from the default context's"
    finally:
        f.close()


def test_chunk_seams_in_a_fresh_process():
    """KOFFT_HIP_SCRATCH_CHUNK_MB=1 in a child process (tests/welch_seams_child.py): 5 rows x 700 frames at win_len 256, so the composed
    route's chunks (about 999 frames) begin and end inside rows; and 3 rows x 800 groups, more partials than the fused route's scratch
    holds at once (2032 groups), so its seams fall inside rows too."""
    env = dict(os.environ, KOFFT_HIP_SCRATCH_CHUNK_MB="1")
    res = subprocess.run([sys.executable, str(ROOT / "tests" / "welch_seams_child.py")], capture_output=True, text=True, timeout=600, env=env,
                         cwd=str(ROOT))
    assert res.returncode == 0 and "seams ok" in res.stdout, res.stdout[-4000:] + res.stderr[-4000:]
