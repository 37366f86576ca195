"""The one-sided STFT (bins 0 .. n/2 of every frame) and its inverse on the device.  Forward: the expected value is always
`oracle.stft(row, win, hop, frames)[:, :K]` per row, bit for bit over every row, on the seam shapes and the route ladder of
tests/test_gpu_stft_rows.py (imported, not copied), every device output pre-filled with NaN.  Inverse: the existing
`istft_rows(..., parallel=True)` on the NumPy-completed frames (tests/onesided_ref.py), and the oracle from a zero output."""
import numpy as np
import pytest

from conftest import bits_equal, seeded
from onesided_ref import ROUND_TRIPS, bins, complete, round_trip_signal
from rowcheck import assert_rows_equal
from test_gpu_stft_rows import SEAM_WINS, _ceil, _dev, _route_cases, _route_shape, _seam_hops, _seam_len, _window

pytestmark = pytest.mark.gpu


def _ref(oracle, x, win, hop, frames):
    k = bins(win.size)
    return np.stack([oracle.stft(r, win, hop, frames)[:, :k] for r in x])


def _onesided_dev(fft, x, stride, win, hop, frames, gap=np.nan, misalign=False, call_stride=None):
    """The device form on rows `stride` apart, the gaps (and nothing else) holding `gap`, the output pre-filled with NaN (misalign: at
    an address that is 8 mod 16; call_stride: the row_stride handed to the call where it is not `stride`); returns [rows, frames, K] complex64."""
    import torch

    rows, length = x.shape
    k = bins(win.size)
    host = np.full((rows, stride), gap, np.float32)
    host[:, :length] = x
    d_sig, d_win = _dev(host.reshape(-1)[:(rows - 1) * stride + length]), _dev(win)
    buf = torch.full((rows * frames * k * 2 + 4,), float("nan"), dtype=torch.float32, device="cuda")
    off = ((8 if misalign else 0) - buf.data_ptr()) % 16 // 4
    out = buf[off:off + rows * frames * k * 2]
    assert out.data_ptr() % 16 == (8 if misalign else 0)
    fft.stft_onesided_dev(d_sig.data_ptr(), rows, length, stride if call_stride is None else call_stride, d_win.data_ptr(), win.size, hop,
                          out.data_ptr(), frames)
    fft.synchronize()
    return out.cpu().numpy().view(np.complex64).reshape(rows, frames, k)


# ---- seams ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win_len", SEAM_WINS)
def test_stft_onesided_seams(fft32, oracle, win_len):
    """rows = 3, row_stride == len: frames at a row's end read +0, never the head of the next row; more frames than ceil(len / hop); then
    row_stride = len + 5 with NaN in the gaps: no NaN anywhere in the NaN-filled output, so every kept bin is written.  Device and host
    forms, and rows = 1."""
    rng = seeded(63000 + win_len)
    win = _window(rng, win_len)
    k = bins(win_len)
    for hop in _seam_hops(win_len):
        length = _seam_len(win_len, hop)
        x = rng.uniform(-1, 1, (3, length)).astype(np.float32)
        req = _ceil(length, hop)
        want = {frames: _ref(oracle, x, win, hop, frames) for frames in (req, req + 2, req + 3)}
        for frames, stride in ((req, length), (req + 3, length), (req, length + 5), (req + 2, length + 5)):
            got = _onesided_dev(fft32, x, stride, win, hop, frames)
            what = f"stft_onesided win {win_len} hop {hop} len {length} frames {frames} stride {stride}"
            assert not np.isnan(got.view(np.float32)).any(), f"{what}: NaN in the output"
            assert_rows_equal(got.reshape(3 * frames, k), want[frames].reshape(3 * frames, k), what)
        assert bits_equal(fft32.stft_onesided(x, win, hop), want[req]), f"host form win {win_len} hop {hop}"
        one = _onesided_dev(fft32, x[1:2], length, win, hop, req, call_stride=0)  # rows = 1: the stride is ignored
        assert bits_equal(one, want[req][1:2]), f"rows = 1, device form, win {win_len} hop {hop}"
        assert bits_equal(fft32.stft_onesided(x[1:2], win, hop, req + 3), want[req + 3][1:2]), f"rows = 1, host form, win {win_len} hop {hop}"


# ---- routes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,frames,rows", _route_cases(), ids=lambda v: str(v))
def test_stft_onesided_routes(fft32, oracle, L, frames, rows):
    """Every small, generic and persistent kernel the one-sided policy instantiates, rows x frames just below and at every dispatch()
    threshold with few, odd frames per row: every kernel walks across many row seams, and a dropped bin that landed in the next frame's
    row of K bins would show as a wrong bin there."""
    n, hop, length = _route_shape(L, frames)
    rng = seeded(64000 + 100 * L + frames)
    win = _window(rng, n)
    x = rng.uniform(-1, 1, (rows, length)).astype(np.float32)
    got = _onesided_dev(fft32, x, length, win, hop, frames)
    k = bins(n)
    assert not np.isnan(got.view(np.float32)).any(), f"n {n} rows {rows} x frames {frames}: NaN in the output"
    assert_rows_equal(got.reshape(rows * frames, k), _ref(oracle, x, win, hop, frames).reshape(rows * frames, k),
                      f"stft_onesided n {n} rows {rows} x frames {frames}")


@pytest.mark.parametrize("L,frames,rows", _route_cases(), ids=lambda v: str(v))
def test_nyquist_row_stays_in_its_row(fft32, oracle, L, frames, rows):
    """Rows (+1, -1, +1, ...) * a carry their energy in bin n/2, the last bin of every K-bin row; the row after each is all zeros.  On
    every route: bin n/2 of the alternating rows is non-zero and equals the oracle's, and the zero rows are zero -- a store of bin n/2
    or of a dropped bin that went one row on would land in them.  (Two distinct rows: two oracle calls.)"""
    n, hop, length = _route_shape(L, frames)
    rng = seeded(65000 + 100 * L + frames)
    win = _window(rng, n)
    alt = (0.75 * (1 - 2 * (np.arange(length) % 2))).astype(np.float32)
    x = np.zeros((rows, length), np.float32)
    x[0::2] = alt
    k = bins(n)
    want_alt, want_zero = (oracle.stft(r, win, hop, frames)[:, :k] for r in (alt, x[1] if rows > 1 else np.zeros(length, np.float32)))
    got = _onesided_dev(fft32, x, length, win, hop, frames)
    assert np.all(got[0::2, 0, n // 2] != 0), "bin n/2 of the alternating rows"
    assert_rows_equal(got[0::2].reshape(-1, k), np.broadcast_to(want_alt, got[0::2].shape).reshape(-1, k), f"alternating rows, n {n}")
    if rows > 1:
        assert not got[1::2].view(np.float32).any(), f"n {n} rows {rows} x frames {frames}: a zero row is not zero"
        assert_rows_equal(got[1::2].reshape(-1, k), np.broadcast_to(want_zero, got[1::2].shape).reshape(-1, k), f"zero rows, n {n}")


# ---- other window lengths -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win_len", [3, 15, 400, 1000])
def test_onesided_non_power_of_two_window(fft32, oracle, win_len):
    """The composed route and the pack kernel; shapes as in test_rows_non_power_of_two_window."""
    rng = seeded(66000 + win_len)
    rows, hop = 5, max(1, (2 * win_len) // 5)
    length = 6 * hop + hop // 2 + 1
    win = _window(rng, win_len)
    x = (rng.uniform(-1, 1, (rows, length)) * (10.0 ** np.arange(rows))[:, None]).astype(np.float32)
    req = _ceil(length, hop)
    k = bins(win_len)
    for frames, stride in ((req, length), (req + 2, length + 5)):
        got = _onesided_dev(fft32, x, stride, win, hop, frames)
        assert_rows_equal(got.reshape(rows * frames, k), _ref(oracle, x, win, hop, frames).reshape(rows * frames, k),
                          f"stft_onesided win {win_len} frames {frames} stride {stride}")
    assert bits_equal(fft32.stft_onesided(x, win, hop), _ref(oracle, x, win, hop, req))


# ---- consistency, alignment -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 1024])
def test_magnitudes_of_the_kept_bins_are_stft_magnitudes(fft32, n):
    """sqrt(re^2 + im^2) in float32 NumPy over bins 0 .. n/2 - 1 of the one-sided result equals stft_magnitudes_rows bit for bit."""
    import kofft_amd

    rng = seeded(66500 + n)
    hop, rows = n // 4, 6
    x = rng.uniform(-1, 1, (rows, 7 * hop - 3)).astype(np.float32)
    half = fft32.stft_onesided(x, kofft_amd.hann(n), hop)[:, :, :n // 2]
    re, im = half.real.astype(np.float32), half.imag.astype(np.float32)
    mags, _ = fft32.stft_magnitudes_rows(x, n, hop)
    assert bits_equal(np.sqrt(re * re + im * im), mags)


@pytest.mark.parametrize("win_len,hop,rows,frames", [(8, 2, 5, 7), (256, 64, 2731, 12), (1024, 256, 1639, 5), (400, 160, 5, 6)])
def test_output_at_an_address_that_is_8_mod_16(fft32, oracle, win_len, hop, rows, frames):
    """Rows of K bins are 8-byte aligned only; two runs give the same bytes, the oracle's."""
    rng = seeded(66700 + win_len)
    length = frames * hop - 1
    win = _window(rng, win_len)
    x = rng.uniform(-1, 1, (rows, length)).astype(np.float32)
    a, b = (_onesided_dev(fft32, x, length, win, hop, frames, misalign=True) for _ in range(2))
    assert bits_equal(a, b)
    k = bins(win_len)
    assert_rows_equal(a.reshape(rows * frames, k), _ref(oracle, x, win, hop, frames).reshape(rows * frames, k), f"win {win_len}, 8 mod 16")


# ---- inverse ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win_len,hop", [(8, 2), (15, 4), (256, 64), (1024, 256), (400, 160), (16, 16), (16, 20)])
def test_istft_onesided(fft32, oracle, win_len, hop):
    """rows = 4, 7 frames of random complex bins, out_len below, at and above the frames' cover, a pre-filled output: the existing
    istft_rows(..., parallel=True) on the NumPy-completed frames; from a zero output also oracle.istft of them (windows in [0.1, 1]: no
    window-square sum is <= 1e-8 where a frame covers).  `half` is unchanged byte for byte.  Host and device forms."""
    rng = seeded(67000 + win_len + hop)
    rows, nfr = 4, 7
    k = bins(win_len)
    win = _window(rng, win_len)
    cover = (nfr - 1) * hop + win_len
    half = (rng.uniform(-1, 1, (rows, nfr, k)) + 1j * rng.uniform(-1, 1, (rows, nfr, k))).astype(np.complex64)
    full = complete(half, win_len)
    d_half, d_win = _dev(half.view(np.float32)), _dev(win)
    for out_len in (cover - hop - 1, cover, cover + 9):
        for pre in (rng.uniform(-1, 1, (rows, out_len)).astype(np.float32), np.zeros((rows, out_len), np.float32)):
            want = pre.copy()
            fft32.istft_rows(full.copy(), win, hop, want, parallel=True)
            if not pre.any():
                ref = np.stack([oracle.istft(full[r].copy(), win, hop, out_len) for r in range(rows)])
                covered = np.zeros(out_len, bool)
                for f in range(nfr):
                    covered[f * hop:f * hop + win_len] = True
                assert bits_equal(want[:, covered], ref[:, covered]) and not want[:, ~covered].any(), f"oracle, out_len {out_len}"
            keep, out = half.copy(), pre.copy()
            fft32.istft_onesided(keep, win, hop, out)
            assert bits_equal(out, want), f"host form, win {win_len} hop {hop} out_len {out_len}"
            assert bits_equal(keep, half), "host form: half was written"
            d_out = _dev(pre)
            fft32.istft_onesided_dev(d_half.data_ptr(), rows, nfr, d_win.data_ptr(), win_len, hop, d_out.data_ptr(), out_len)
            fft32.synchronize()
            assert bits_equal(d_out.cpu().numpy(), want), f"device form, win {win_len} hop {hop} out_len {out_len}"
    assert bits_equal(d_half.cpu().numpy().view(np.complex64).reshape(half.shape), half), "device form: half was written"


@pytest.mark.parametrize("win_len,hop,seed", ROUND_TRIPS)
def test_round_trip(fft32, oracle, win_len, hop, seed):
    """Hann windows, len = 9 * hop + 17: the largest absolute error of istft_onesided(stft_onesided(x)) on the samples at least win_len
    from either end is at most twice that of the oracle's full round trip on the same signal (with the oracle alone the ratio lies
    between 0.98 and 1.21 over six shapes; tests/test_stft_onesided_cpu.py holds these three to the bound without a device)."""
    import kofft_amd

    x = round_trip_signal(win_len, hop, seed)
    win = kofft_amd.hann(win_len)
    length = x.size
    frames = _ceil(length, hop)
    half = fft32.stft_onesided(x[None, :], win, hop)
    out = np.zeros((1, length), np.float32)
    fft32.istft_onesided(half, win, hop, out)
    ref = oracle.istft(oracle.stft(x, win, hop, frames), win, hop, length)
    mid = slice(win_len, length - win_len)
    err, err_ref = float(np.abs(out[0, mid] - x[mid]).max()), float(np.abs(ref[mid] - x[mid]).max())
    print(f"win {win_len} hop {hop}: one-sided {err:.3e} oracle {err_ref:.3e} ratio {err / err_ref:.3f}")
    assert err <= 2 * err_ref


# ---- switches -----------------------------------------------------------------------------------------------------------------------
def test_onesided_generic_kernel_at_32_points(oracle, monkeypatch):
    """KOFFT_HIP_SMALL32=0 in a fresh context: n = 32 runs the generic kernel instead of the one-thread-per-transform one (the one
    instantiation of the one-sided policy the default routes never reach)."""
    import kofft_amd

    monkeypatch.setenv("KOFFT_HIP_SMALL32", "0")
    plain = kofft_amd.HipFftImpl(np.float32)
    try:
        rng = seeded(66900)
        n, hop, rows, frames = 32, 8, 41, 5
        win = _window(rng, n)
        x = rng.uniform(-1, 1, (rows, frames * hop - 3)).astype(np.float32)
        got = _onesided_dev(plain, x, x.shape[1], win, hop, frames)
        assert_rows_equal(got.reshape(rows * frames, bins(n)), _ref(oracle, x, win, hop, frames).reshape(rows * frames, bins(n)),
                          "stft_onesided n 32, generic kernel")
    finally:
        plain.close()
