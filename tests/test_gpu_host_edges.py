"""Degenerate shapes through the host-pointer entry points, on both routes of the host staging path: once in a context
that may go zero-copy and once in one created with KOFFT_HIP_ZERO_COPY=0 (every call staged).  The two results must be the same
bytes, and the oracle's where the oracle defines the case: empty arrays, frames that see no sample, outputs of length 0."""
import os

import numpy as np
import pytest

import kofft_amd as K
from kofft_amd.api import _ptr
from conftest import bits_equal, rand_c, seeded

pytestmark = pytest.mark.gpu

WINDOWS = (8, 64)


@pytest.fixture(scope="module")
def routes():
    """(zero-copy allowed, always staged): the variable is read when the context is created."""
    saved = os.environ.pop("KOFFT_HIP_ZERO_COPY", None)
    try:
        plain = K.HipFftImpl(np.float32)
        os.environ["KOFFT_HIP_ZERO_COPY"] = "0"
        staged = K.HipFftImpl(np.float32)
    finally:
        os.environ.pop("KOFFT_HIP_ZERO_COPY", None)
        if saved is not None:
            os.environ["KOFFT_HIP_ZERO_COPY"] = saved
    yield plain, staged
    plain.close()
    staged.close()


def on_both(routes, call, what):
    """call(fft) -> tuple of arrays, in each context; the same bytes from both; returns the first."""
    a, b = call(routes[0]), call(routes[1])
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert bits_equal(np.asarray(x), np.asarray(y)), f"{what}: result {i} differs between the zero-copy and the staged route"
    return a


def _win(n):
    return seeded(40 + n).uniform(0.1, 1, n).astype(np.float32)


@pytest.mark.parametrize("win_len", WINDOWS)
def test_stft_frame_that_starts_past_the_signal(routes, oracle, win_len):
    sig = seeded(1).uniform(-1, 1, 20).astype(np.float32)
    win = _win(win_len)
    zeros = oracle.fft(np.zeros((1, win_len), np.complex64))[0]
    for start in (20, 27):
        def call(f):
            out = rand_c(seeded(2), win_len)
            f.stft_frame(sig, win, start, out)
            return (out,)
        (out,) = on_both(routes, call, f"stft_frame start={start}")
        assert bits_equal(out, oracle.stft_range(sig, win, 1, start, 1)[0]) and bits_equal(out, zeros)


@pytest.mark.parametrize("win_len", WINDOWS)
def test_stft_of_an_empty_signal(routes, oracle, win_len):
    win = _win(win_len)
    want = oracle.stft(np.zeros(0, np.float32), win, 3, 2)
    assert bits_equal(want, oracle.fft(np.zeros((2, win_len), np.complex64)))
    (one,) = on_both(routes, lambda f: (f.stft_into(np.zeros(0, np.float32), win, 3, 2),), "stft_into len=0")
    assert bits_equal(one, want)
    (rows,) = on_both(routes, lambda f: (f.stft_rows(np.zeros((3, 0), np.float32), win, 3, 2),), "stft_rows len=0")
    assert rows.shape == (3, 2, win_len)
    for r in rows:
        assert bits_equal(r, want)


@pytest.mark.parametrize("win_len", WINDOWS)
def test_stft_rows_with_a_row_stride_above_len(routes, win_len):
    rows, length, stride, hop = 3, 37, 50, 5
    frames = -(-length // hop)
    buf = seeded(3).uniform(-1, 1, (rows, stride)).astype(np.float32)
    win = _win(win_len)

    def call(f):
        out = np.zeros((rows, frames, win_len), np.complex64)
        f._check(f._lib.kofft_hip_stft_rows_f32(f._ctx, _ptr(buf), rows, length, stride, _ptr(win), win_len, hop, _ptr(out), frames))
        return (out,)
    (out,) = on_both(routes, call, "stft_rows stride")
    for r in range(rows):
        assert bits_equal(out[r], routes[0].stft_into(np.ascontiguousarray(buf[r, :length]), win, hop, frames)), f"row {r}"


@pytest.mark.parametrize("win_len", WINDOWS)
def test_istft_without_frames(routes, win_len):
    """istft_ola_kernel / istft_ola_rows_kernel with no frame: every window-square sum is 0, so the output keeps what it held (istft) or
    becomes 0 (inverse_parallel), and the scratch is 0."""
    win = _win(win_len)
    prior = seeded(4).uniform(-1, 1, (3, 40)).astype(np.float32)

    def single(f):
        out, scr = prior[0].copy(), np.full(40, 7.0, np.float32)
        f.istft_contiguous(np.zeros((0, win_len), np.complex64), win, 2, out, scr)
        par = prior[0].copy()
        K.inverse_parallel(np.zeros((0, win_len), np.complex64), win, 2, par, f)
        return out, scr, par
    out, scr, par = on_both(routes, single, "istft frames=0")
    assert bits_equal(out, prior[0]) and bits_equal(scr, np.zeros(40, np.float32)) and bits_equal(par, np.zeros(40, np.float32))

    def rowwise(f):
        out, scr = prior.copy(), np.full((3, 40), 7.0, np.float32)
        f.istft_rows(np.zeros((3, 0, win_len), np.complex64), win, 2, out, scr)
        par = prior.copy()
        f.istft_rows(np.zeros((3, 0, win_len), np.complex64), win, 2, par, parallel=True)
        return out, scr, par
    out, scr, par = on_both(routes, rowwise, "istft_rows frames=0")
    assert bits_equal(out, prior) and bits_equal(scr, np.zeros((3, 40), np.float32)) and bits_equal(par, np.zeros((3, 40), np.float32))


@pytest.mark.parametrize("win_len", WINDOWS)
def test_istft_into_an_empty_output(routes, oracle, win_len):
    frames = rand_c(seeded(5), (3, win_len))
    win = _win(win_len)

    def call(f):
        fr = frames.copy()
        f.istft_contiguous(fr, win, 2, np.zeros(0, np.float32), np.zeros(0, np.float32))
        return (fr,)
    (fr,) = on_both(routes, call, "istft out_len=0")
    assert bits_equal(fr, oracle.ifft(frames))


def test_istft_rows_of_one_row_is_the_single_call(routes):
    win_len, hop, nfr = 64, 16, 5
    out_len = (nfr - 1) * hop + win_len
    frames = rand_c(seeded(6), (nfr, win_len))
    win = _win(win_len)
    prior = seeded(7).uniform(-1, 1, out_len).astype(np.float32)

    def call(f):
        fr1, out1, scr1 = frames.copy(), prior.copy(), np.zeros(out_len, np.float32)
        f.istft_contiguous(fr1, win, hop, out1, scr1)
        frr, outr, scrr = frames.copy()[None], prior.copy()[None], np.zeros((1, out_len), np.float32)
        f.istft_rows(frr, win, hop, outr, scrr)
        assert bits_equal(frr[0], fr1) and bits_equal(outr[0], out1) and bits_equal(scrr[0], scr1), "mode 1"
        fr2, out2 = frames.copy(), prior.copy()
        K.inverse_parallel(fr2, win, hop, out2, f)
        frp, outp = frames.copy()[None], prior.copy()[None]
        f.istft_rows(frp, win, hop, outp, parallel=True)
        assert bits_equal(frp[0], fr2) and bits_equal(fr2, frames) and bits_equal(outp[0], out2), "mode 2"
        return fr1, out1, scr1, out2
    on_both(routes, call, "istft_rows rows=1")


@pytest.mark.parametrize("win_len", WINDOWS)
def test_inverse_frame_that_runs_past_the_output(routes, oracle, win_len):
    """stft::inverse_frame (stft.rs:393-397) adds only where start + i < output.len(): a frame past the end is cut, not an error --
    istft_ola_kernel<0> returns for s >= out_len."""
    out_len = 30
    frame = rand_c(seeded(8), win_len)
    win = _win(win_len)
    prior = seeded(9).uniform(-1, 1, out_len).astype(np.float32)
    time = oracle.ifft(frame[None])[0]
    for start in (out_len - 3, out_len + 2):
        def call(f):
            fr, out = frame.copy(), prior.copy()
            K.inverse_frame(fr, win, start, out, f)
            return fr, out
        fr, out = on_both(routes, call, f"inverse_frame start={start}")
        want = prior.copy()
        have = max(0, out_len - start)
        want[start:] = want[start:] + time.real[:have] * win[:have]
        assert bits_equal(fr, time) and bits_equal(out, want)


def test_stft_magnitudes_without_samples_or_bins(routes, oracle):
    for win_len in WINDOWS:  # no samples: no frames, the maximum stays 0
        mags, mx = on_both(routes, lambda f: f.stft_magnitudes(np.zeros(0, np.float32), win_len, 2), "stft_magnitudes len=0")
        assert mags.shape == (0, win_len // 2) and mx == 0.0
        mags, mx = on_both(routes, lambda f: f.stft_magnitudes_rows(np.zeros((3, 0), np.float32), win_len, 2), "stft_magnitudes_rows len=0")
        assert mags.shape == (3, 0, win_len // 2) and bits_equal(mx, np.zeros(3, np.float32))
    x = seeded(10).uniform(-1, 1, (3, 10)).astype(np.float32)  # a one-sample window: frames, but no bin below win_len / 2
    mags, mx = on_both(routes, lambda f: f.stft_magnitudes(x[0], 1, 2), "stft_magnitudes win_len=1")
    wm, wmx = oracle.stft_magnitudes(x[0], 1, 2)
    assert mags.shape == wm.shape == (5, 0) and mx == wmx == 0.0
    mags, mx = on_both(routes, lambda f: f.stft_magnitudes_rows(x, 1, 2), "stft_magnitudes_rows win_len=1")
    assert mags.shape == (3, 5, 0) and bits_equal(mx, np.zeros(3, np.float32))


def test_entries_that_never_go_zero_copy(routes, oracle):
    x = rand_c(seeded(11), (3, 16))

    def radix4(f):
        y = x.copy()
        f.fft_radix4_batch(y)
        return (y,)
    (y,) = on_both(routes, radix4, "fft_radix4_batch")
    assert bits_equal(y, oracle.fft_radix4(x))
    vol = rand_c(seeded(12), 2 * 4 * 8)

    def nd(f):
        v = vol.copy()
        f.fftnd(v, 2, 4, 8)
        return (v,)
    on_both(routes, nd, "fftnd")
