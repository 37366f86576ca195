"""STFT, stft_magnitudes and ISTFT over rows of signals on the device.  The expected value is always the oracle applied
per row (or, for the ISTFT side effects the oracle does not return, the single-signal entry per row); every comparison is bit for bit and
covers every row.  Shapes are the smallest at which a row seam can go wrong: len no multiple of hop and below win + hop (the last frames
of every row zero-pad), row_stride == len (the next row's head lies directly behind), a NaN gap when row_stride > len, and rows x frames
just below and just above every dispatch() threshold of a 256-CU part with few, odd frames per row."""
import numpy as np
import pytest

from conftest import bits_equal, seeded
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ceil(a, b):
    return -(-a // b)


def _window(rng, n):
    return rng.uniform(0.1, 1.0, n).astype(np.float32)


def _stft_ref(oracle, x, win, hop, frames):
    return np.stack([oracle.stft(r, win, hop, frames) for r in x]) if len(x) else np.zeros((0, frames, win.size), np.complex64)


def _mag_ref(oracle, x, win_len, hop):
    res = [oracle.stft_magnitudes(r, win_len, hop) for r in x]
    return np.stack([m for m, _ in res]), np.array([mx for _, mx in res], np.float32)


def _stft_rows_dev(fft, x, stride, win, hop, frames, gap=np.nan):
    """The device form on rows `stride` apart, the gaps (and nothing else) holding `gap`; returns [rows, frames, win] complex64."""
    import torch

    rows, length = x.shape
    host = np.full((rows, stride), gap, np.float32)
    host[:, :length] = x
    d_sig, d_win = _dev(host.reshape(-1)[:(rows - 1) * stride + length] if rows else host.reshape(-1)), _dev(win)
    out = torch.full((rows, frames, win.size, 2), float("nan"), dtype=torch.float32, device="cuda")
    fft.stft_rows_dev(d_sig.data_ptr(), rows, length, stride, d_win.data_ptr(), win.size, hop, out.data_ptr(), frames)
    fft.synchronize()
    return out.cpu().numpy().view(np.complex64).reshape(rows, frames, win.size)


def _mag_rows_dev(fft, x, stride, win_len, hop, frames, gap=np.nan):
    import torch

    rows, length = x.shape
    host = np.full((rows, stride), gap, np.float32)
    host[:, :length] = x
    d_sig = _dev(host.reshape(-1)[:(rows - 1) * stride + length])
    mags = torch.full((rows, frames, win_len // 2), float("nan"), dtype=torch.float32, device="cuda")
    mx = torch.full((rows,), float("nan"), dtype=torch.float32, device="cuda")
    fft.stft_magnitudes_rows_dev(d_sig.data_ptr(), rows, length, stride, win_len, hop, mags.data_ptr(), frames, mx.data_ptr())
    fft.synchronize()
    return mags.cpu().numpy(), mx.cpu().numpy()


SEAM_WINS = [1, 2, 16, 32, 64, 256, 1024, 4096, 8192, 16384]


def _seam_hops(win):
    return sorted({1, max(1, win // 4), win, win + 3})


def _seam_len(win, hop):
    """Not a multiple of hop, below win + hop, and long enough for at least three frames: the last two or three zero-pad.  hop = 1 divides
    every length, so there the row is short instead (at most 7 samples, below win + 1): every frame of it runs past the row's end, with the
    next row's head directly behind, and every window length runs hop = 1 in kilobytes."""
    if hop == 1:
        return min(win, 7)
    length = min(win + hop - 1, max(2 * hop + 1, win // 2 + 1))
    if length % hop == 0:
        length -= 1
    return max(length, 1)


# ---- seams ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win_len", SEAM_WINS)
def test_stft_rows_seams(fft32, oracle, win_len):
    """rows = 3, row_stride == len: frames at a row's end read +0, never the head of the next row.  Then more frames than ceil(len / hop)
    (whole frames of zeros at each row's end), then row_stride = len + 5 with NaN in the gaps: no NaN anywhere in the output."""
    rng = seeded(51000 + win_len)
    win = _window(rng, win_len)
    for hop in _seam_hops(win_len):
        length = _seam_len(win_len, hop)
        x = rng.uniform(-1, 1, (3, length)).astype(np.float32)
        req = _ceil(length, hop)
        for frames, stride in ((req, length), (req + 3, length), (req, length + 5), (req + 2, length + 5)):
            got = _stft_rows_dev(fft32, x, stride, win, hop, frames)
            assert not np.isnan(got.view(np.float32)).any(), f"win {win_len} hop {hop} frames {frames} stride {stride}: NaN in the output"
            assert_rows_equal(got.reshape(3 * frames, -1), _stft_ref(oracle, x, win, hop, frames).reshape(3 * frames, -1),
                              f"stft_rows win {win_len} hop {hop} len {length} frames {frames} stride {stride}")
        # host form, same rows
        assert bits_equal(fft32.stft_rows(x, win, hop), _stft_ref(oracle, x, win, hop, req)), f"host form win {win_len} hop {hop}"


@pytest.mark.parametrize("win_len", SEAM_WINS)
def test_magnitudes_rows_seams(fft32, oracle, win_len):
    """The same seams for the magnitudes: rows scaled by 10**r, so a maximum that leaks from a neighbour shows; whole frames of zeros beyond
    ceil(len / hop) give +0 magnitudes and leave the maxima alone."""
    rng = seeded(52000 + win_len)
    for hop in _seam_hops(win_len):
        length = _seam_len(win_len, hop)
        req = _ceil(length, hop)
        x = (rng.uniform(-1, 1, (3, length)) * (10.0 ** np.arange(3))[:, None]).astype(np.float32)
        want_m, want_x = _mag_ref(oracle, x, win_len, hop)
        for frames, stride in ((req, length), (req + 3, length), (req, length + 5)):
            mags, mx = _mag_rows_dev(fft32, x, stride, win_len, hop, frames)
            what = f"magnitudes_rows win {win_len} hop {hop} len {length} frames {frames} stride {stride}"
            assert not np.isnan(mags).any() and not np.isnan(mx).any(), what
            assert_rows_equal(mags[:, :req].reshape(3 * req, -1), want_m.reshape(3 * req, -1), what)
            assert bits_equal(mags[:, req:], np.zeros_like(mags[:, req:])), what + ": frames of zeros"
            assert bits_equal(mx, want_x), f"{what}: max {mx} want {want_x}"
        hm, hx = fft32.stft_magnitudes_rows(x, win_len, hop)
        assert bits_equal(hm, want_m) and bits_equal(hx, want_x), f"host form win {win_len} hop {hop}"


# ---- routes -----------------------------------------------------------------------------------------------------------------------
# dispatch() (host_common.hip.h) on a 256-CU part: the persistent kernels start at CUs x k transforms
THRESH = {6: 256 * 512, 7: 256 * 256, 8: 256 * 128, 9: 256 * 64, 10: 256 * 32, 11: 256 * 16, 12: 256 * 4, 13: 256 * 4}
SMALL = (1, 2, 3, 4, 5)  # log2 n of fft_small_kernel (n = 32 too): several workgroups, a ragged last one


def _route_cases():
    cases = []
    for L in SMALL:
        cases += [(L, 5, 1031), (L, 129, 41), (L, 256, 3)]  # (256 frames: the workgroup descriptor form, a multiple of every block)
    for L, t in THRESH.items():
        cases += [(L, 5, t // 5), (L, 5, t // 5 + 1)]  # just below / at or above the threshold, five frames per row
        if L <= 8:
            cases.append((L, 12, t // 12 + 1))  # groups of 2 / 4 frames stay inside a row: the persistent group kernels
        if L in (9, 10):
            cases.append((L, 129, t // 129 + 1))
    cases += [(L, 16, 5) for L in range(5, 13)]  # frames a multiple of the generic kernels' tile: their one-descriptor-per-workgroup loads
    cases += [(14, 5, 7), (14, 4, 3)]  # n = 16384: the generic kernel at every batch (the wave-split kernels are not taken)
    return cases


def _route_shape(L, frames):
    n = 1 << L
    hop = max(1, n // 4)
    return n, hop, frames * hop - min(3, hop - 1) if hop > 1 else frames  # frames == ceil(len / hop), the last frames zero-pad


@pytest.mark.parametrize("L,frames,rows", _route_cases(), ids=lambda v: str(v))
def test_stft_rows_routes(fft32, oracle, L, frames, rows):
    """Every small, generic, persistent kernel the row policies instantiate, with rows x frames around its threshold and the total made of
    MANY rows: every kernel walks across many seams, rows and frames no multiple of a tile width."""
    n, hop, length = _route_shape(L, frames)
    rng = seeded(53000 + 100 * L + frames)
    win = _window(rng, n)
    x = rng.uniform(-1, 1, (rows, length)).astype(np.float32)
    got = fft32.stft_rows(x, win, hop)
    assert got.shape == (rows, frames, n)
    assert_rows_equal(got.reshape(rows * frames, n), _stft_ref(oracle, x, win, hop, frames).reshape(rows * frames, n),
                      f"stft_rows n {n} rows {rows} x frames {frames}")


@pytest.mark.parametrize("L,frames,rows", _route_cases(), ids=lambda v: str(v))
def test_magnitudes_rows_routes(fft32, oracle, L, frames, rows):
    """The same ladder for the magnitudes; rows scaled by 10**(r % 7 - 3), one all-zero row (maximum 0.0), one row with a NaN sample (NaNs in
    the same places, its maximum ignores them, its neighbours are unaffected)."""
    n, hop, length = _route_shape(L, frames)
    rng = seeded(54000 + 100 * L + frames)
    x = (rng.uniform(-1, 1, (rows, length)) * (10.0 ** (np.arange(rows) % 7 - 3))[:, None]).astype(np.float32)
    zero_row, nan_row = rows // 2, min(rows - 1, rows // 2 + 1)
    x[zero_row] = 0.0
    if nan_row != zero_row:
        x[nan_row, length // 2] = np.nan
    mags, mx = fft32.stft_magnitudes_rows(x, n, hop)
    want_m, want_x = _mag_ref(oracle, x, n, hop)
    what = f"magnitudes_rows n {n} rows {rows} x frames {frames}"
    assert_rows_equal(mags.reshape(rows * frames, -1), want_m.reshape(rows * frames, -1), what, nan_safe=True)
    assert bits_equal(mx, want_x), f"{what}: maxima differ at rows {np.flatnonzero(mx.view(np.uint32) != want_x.view(np.uint32))[:8]}"
    assert mx[zero_row] == 0.0 and not np.isnan(mx).any()


# ---- other window lengths -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win_len", [3, 400, 1000])
def test_rows_non_power_of_two_window(fft32, oracle, win_len):
    rng = seeded(55000 + win_len)
    rows, hop = 5, max(1, (2 * win_len) // 5)
    length = 6 * hop + hop // 2 + 1
    win = _window(rng, win_len)
    x = (rng.uniform(-1, 1, (rows, length)) * (10.0 ** np.arange(rows))[:, None]).astype(np.float32)
    req = _ceil(length, hop)
    for frames, stride in ((req, length), (req + 2, length + 5)):
        got = _stft_rows_dev(fft32, x, stride, win, hop, frames)
        assert_rows_equal(got.reshape(rows * frames, -1), _stft_ref(oracle, x, win, hop, frames).reshape(rows * frames, -1),
                          f"stft_rows win {win_len} frames {frames} stride {stride}")
    assert bits_equal(fft32.stft_rows(x, win, hop), _stft_ref(oracle, x, win, hop, req))
    want_m, want_x = _mag_ref(oracle, x, win_len, hop)
    for stride in (length, length + 5):
        mags, mx = _mag_rows_dev(fft32, x, stride, win_len, hop, req)
        assert_rows_equal(mags.reshape(rows * req, -1), want_m.reshape(rows * req, -1), f"magnitudes_rows win {win_len} stride {stride}")
        assert bits_equal(mx, want_x), f"win {win_len}: max {mx} want {want_x}"
    hm, hx = fft32.stft_magnitudes_rows(x, win_len, hop)
    assert bits_equal(hm, want_m) and bits_equal(hx, want_x)


# ---- ISTFT --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win_len,hop", [(8, 2), (256, 64), (1024, 256), (400, 160), (16, 16), (16, 20)])
def test_istft_rows_both_modes(fft32, oracle, win_len, hop):
    """rows = 4, out_len shorter than, equal to and longer than the frames cover.  Mode 1: a pre-filled output is accumulated into, scratch
    holds the per-row window-square sums, the frames hold their inverse transforms; mode 2: the frames are unchanged.  Expected: the
    single-signal entry per row (and the oracle for mode 1's output from zero), host and device forms."""
    import kofft_amd

    rng = seeded(56000 + win_len + hop)
    rows, nfr = 4, 7
    win = _window(rng, win_len)
    cover = (nfr - 1) * hop + win_len
    spec = (rng.uniform(-1, 1, (rows, nfr, win_len)) + 1j * rng.uniform(-1, 1, (rows, nfr, win_len))).astype(np.complex64)
    for out_len in (cover - hop - 1, cover, cover + 9):
        pre = rng.uniform(-1, 1, (rows, out_len)).astype(np.float32)
        # mode 1, single-signal references
        want_fr, want_out, want_scr = spec.copy(), pre.copy(), np.zeros((rows, out_len), np.float32)
        for r in range(rows):
            fft32.istft_contiguous(want_fr[r], win, hop, want_out[r], want_scr[r])
        zero_out = np.zeros((rows, out_len), np.float32)
        fr0 = spec.copy()
        fft32.istft_rows(fr0, win, hop, zero_out, np.zeros_like(zero_out))
        assert bits_equal(zero_out, np.stack([oracle.istft(spec[r], win, hop, out_len) for r in range(rows)])), f"oracle, out_len {out_len}"
        fr, out, scr = spec.copy(), pre.copy(), np.full((rows, out_len), np.nan, np.float32)
        fft32.istft_rows(fr, win, hop, out, scr)
        assert bits_equal(out, want_out) and bits_equal(scr, want_scr) and bits_equal(fr, want_fr), f"host mode 1, out_len {out_len}"
        d_fr, d_out, d_scr, d_win = _dev(spec.view(np.float32)), _dev(pre), _dev(np.full((rows, out_len), np.nan, np.float32)), _dev(win)
        fft32.istft_rows_dev(d_fr.data_ptr(), rows, nfr, d_win.data_ptr(), win_len, hop, d_out.data_ptr(), out_len, d_scr.data_ptr())
        fft32.synchronize()
        assert bits_equal(d_out.cpu().numpy(), want_out) and bits_equal(d_scr.cpu().numpy(), want_scr), f"device mode 1, out_len {out_len}"
        assert bits_equal(d_fr.cpu().numpy().view(np.complex64).reshape(spec.shape), want_fr), "device mode 1: the frames' inverse transforms"
        # mode 2
        want2 = pre.copy()
        for r in range(rows):
            kofft_amd.inverse_parallel(spec[r], win, hop, want2[r], fft32)
        fr, out = spec.copy(), pre.copy()
        fft32.istft_rows(fr, win, hop, out, parallel=True)
        assert bits_equal(out, want2) and bits_equal(fr, spec), f"host mode 2, out_len {out_len}"
        d_fr, d_out = _dev(spec.view(np.float32)), _dev(pre)
        fft32.istft_rows_dev(d_fr.data_ptr(), rows, nfr, d_win.data_ptr(), win_len, hop, d_out.data_ptr(), out_len, parallel=True)
        fft32.synchronize()
        assert bits_equal(d_out.cpu().numpy(), want2), f"device mode 2, out_len {out_len}"
        assert bits_equal(d_fr.cpu().numpy().view(np.complex64).reshape(spec.shape), spec), "device mode 2: the frames are unchanged"


@pytest.mark.parametrize("win_len,hop", [(256, 64), (400, 160), (1024, 256)])
def test_round_trip_rows_equals_single_signal(fft32, oracle, win_len, hop):
    import kofft_amd

    rng = seeded(57000 + win_len)
    rows, length = 4, 9 * hop + 17
    win = kofft_amd.hann(win_len)
    x = rng.uniform(-1, 1, (rows, length)).astype(np.float32)
    frames = _ceil(length, hop)
    spec = fft32.stft_rows(x, win, hop)
    out, scr = np.zeros((rows, length), np.float32), np.zeros((rows, length), np.float32)
    fft32.istft_rows(spec.copy(), win, hop, out, scr)
    for r in range(rows):
        one = fft32.stft_into(x[r], win, hop, frames)
        assert bits_equal(one, spec[r])
        o1, s1 = np.zeros(length, np.float32), np.zeros(length, np.float32)
        fft32.istft_contiguous(one, win, hop, o1, s1)
        assert bits_equal(out[r], o1) and bits_equal(scr[r], s1), f"row {r}"
    # and to the oracle's round trip (how close that comes to x is the reference's own business: its Bluestein arm at 400 points
    # reconstructs to about 1e-4, the power-of-two windows to about 1e-6)
    assert bits_equal(out, np.stack([oracle.istft(oracle.stft(x[r], win, hop, frames), win, hop, length) for r in range(rows)]))


# ---- equivalences -------------------------------------------------------------------------------------------------------------------
def _loop_stft(fft, x, win, hop, frames):
    return np.stack([fft.stft_into(r, win, hop, frames) for r in x])


@pytest.mark.parametrize("win_len,hop,rows,length", [(512, 128, 7, 1601), (1024, 256, 33, 48001), (400, 160, 9, 4801), (64, 16, 1, 999)])
def test_rows_call_equals_loop_of_single_calls(fft32, win_len, hop, rows, length):
    """Device forms and host forms (zero-copy size and staged size) against the existing single-signal call per row, byte for byte;
    rows = 1 equals the existing entry; two runs give the same bytes."""
    import kofft_amd

    rng = seeded(58000 + win_len + rows)
    win = kofft_amd.hann(win_len)
    x = rng.uniform(-1, 1, (rows, length)).astype(np.float32)
    frames = _ceil(length, hop)
    want = _loop_stft(fft32, x, win, hop, frames)
    host = fft32.stft_rows(x, win, hop)
    assert bits_equal(host, want) and bits_equal(fft32.stft_rows(x, win, hop), host)
    assert bits_equal(_stft_rows_dev(fft32, x, length, win, hop, frames), want)
    mags, mx = fft32.stft_magnitudes_rows(x, win_len, hop)
    singles = [fft32.stft_magnitudes(r, win_len, hop) for r in x]
    assert bits_equal(mags, np.stack([m for m, _ in singles])) and bits_equal(mx, np.array([v for _, v in singles], np.float32))
    m2, x2 = _mag_rows_dev(fft32, x, length, win_len, hop, frames)
    assert bits_equal(m2, mags) and bits_equal(x2, mx)


def test_magnitudes_rows_of_long_rows(fft32, oracle):
    """Rows that reach the persistent kernels on their own (n = 1024: 8192 frames and more) run the single-signal kernel row by row:
    the same bytes, one maximum per row, the seam between the two rows intact."""
    rng = seeded(58500)
    rows, frames, n, hop = 2, 8193, 1024, 256
    x = (rng.uniform(-1, 1, (rows, frames * hop - 3)) * np.array([[1.0], [100.0]])).astype(np.float32)
    mags, mx = fft32.stft_magnitudes_rows(x, n, hop)
    want_m, want_x = _mag_ref(oracle, x, n, hop)
    assert_rows_equal(mags.reshape(rows * frames, -1), want_m.reshape(rows * frames, -1), "magnitudes_rows 2 x 8193 frames")
    assert bits_equal(mx, want_x)


def test_pipelined_host_call_equals_loop(oracle, monkeypatch):
    """256 clips of 16 000 samples at 512 / 128: 144 MiB through the host pipeline (whole rows per chunk), in a fresh context."""
    import kofft_amd

    monkeypatch.setenv("KOFFT_HIP_HOST_PIPELINE", "1")
    fft = kofft_amd.HipFftImpl(np.float32)
    try:
        rng = seeded(59000)
        rows, length, win_len, hop = 256, 16000, 512, 128
        win = kofft_amd.hann(win_len)
        x = rng.uniform(-1, 1, (rows, length)).astype(np.float32)
        got = fft.stft_rows(x, win, hop)
        assert got.nbytes + x.nbytes >= 128 << 20
        for r in (0, 1, 31, 32, 33, 127, 128, 255):  # chunk seams of the eight-piece pipeline, every chunk
            assert bits_equal(got[r], oracle.stft(x[r], win, hop, 125)), f"row {r}"
        assert bits_equal(got, _loop_stft(fft, x, win, hop, 125))
    finally:
        fft.close()


# ---- switches -----------------------------------------------------------------------------------------------------------------------
def test_rows_without_the_persistent_kernels(fft32, monkeypatch):
    """KOFFT_HIP_NO_PERSIST=1 in a fresh context: the generic kernels give the same bytes as the persistent ones."""
    import kofft_amd

    rng = seeded(60000)
    monkeypatch.setenv("KOFFT_HIP_NO_PERSIST", "1")
    plain = kofft_amd.HipFftImpl(np.float32)
    try:
        for n, frames in ((64, 12), (512, 5), (1024, 5), (4096, 5)):
            hop = n // 4
            rows = THRESH[n.bit_length() - 1] // frames + 1
            length = frames * hop - 3
            x = (rng.uniform(-1, 1, (rows, length)) * (10.0 ** (np.arange(rows) % 5))[:, None]).astype(np.float32)
            win = kofft_amd.hann(n)
            assert bits_equal(plain.stft_rows(x, win, hop), fft32.stft_rows(x, win, hop)), f"stft_rows n {n}"
            (m0, x0), (m1, x1) = plain.stft_magnitudes_rows(x, n, hop), fft32.stft_magnitudes_rows(x, n, hop)
            assert bits_equal(m0, m1) and bits_equal(x0, x1), f"magnitudes_rows n {n}"
    finally:
        plain.close()
