"""Rows of audio to mel energies / MFCCs in one call (kofft_hip_stft_mel_f32, kofft_hip_stft_mfcc_f32 and their kofft_hip_dev_* forms)
against the two existing oracles composed (tests/frontend_oracle.py: oracle.stft_magnitudes, then tests/mel_oracle.py), every frame
of every row bit for bit, NaNs by position.  Every case runs on the default context, on the composed route (set_frontend_fused(0):
magnitudes into the context's scratch, then the mel / MFCC path) and on the fused kernel wherever it fits (set_frontend_fused(2):
power-of-two windows of 64 .. 2048 samples, up to 128 filters; everything else is composed there too).

Shapes: the fused kernel carries XPB = 16 frames per workgroup at win_len 64 .. 256, 4 at 512 and 1024, 2 at 2048, over the flat index
row * frames + frame; its loads take one descriptor per workgroup only where XPB divides `frames` and the hop is small.  Kernel
instances and the tests that launch them are listed in DESIGN.md 5.23."""
import ctypes as C

import numpy as np
import pytest

import frontend_oracle as fo
import mel_oracle as mo
from conftest import bits_equal, seeded
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32
XPB = {64: 16, 128: 16, 256: 16, 512: 4, 1024: 4, 2048: 2}
KNOB = "KOFFT_HIP_SCRATCH_CHUNK_MB"


@pytest.fixture(scope="module")
def composed32():
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_frontend_fused(0)
    yield f
    f.close()


@pytest.fixture(scope="module")
def forced32():
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_frontend_fused(2)
    yield f
    f.close()


def _ref_bins(rate, n_fft, filters):
    from kofft_amd import mfcc

    return [int(b) for b in mfcc.mel_bins(float(rate), n_fft, filters)]


def _counts(num_mel):
    return sorted({min(1, num_mel), min(13, num_mel), num_mel})


def _check_all(ctxs, oracle, x, win_len, hop, frames, bins, what, window=None, counts=None):
    """Energies and coefficients of the host forms on every context against the oracle, every frame of every row."""
    num_mel = len(bins) - 2
    want_e, want_c = fo.expected(oracle, x, win_len, hop, frames, bins, window)
    for name, f in ctxs:
        got_e = f.stft_mel_rows(x, win_len, hop, bins, window, frames)
        assert got_e.shape == want_e.shape
        assert_rows_equal(got_e.reshape(-1, num_mel), want_e.reshape(-1, num_mel), f"{what}: energies, {name}", nan_safe=True)
        for nc in counts or _counts(num_mel):
            got = f.stft_mfcc_rows(x, win_len, hop, bins, nc, window, frames)
            want = np.ascontiguousarray(want_c[:, :, :nc])
            assert_rows_equal(got.reshape(-1, nc), want.reshape(-1, nc), f"{what} nc={nc}: coefficients, {name}", nan_safe=True)
    return want_e, want_c


@pytest.fixture()
def ctxs(fft32, composed32, forced32):
    return [("default", fft32), ("set_frontend_fused(0)", composed32), ("set_frontend_fused(2)", forced32)]


@pytest.mark.parametrize("win_len", [32, 64, 128, 256, 1024, 2048, 4096])
def test_small_shapes_around_the_workgroup_tile(ctxs, oracle, win_len):
    """frames one below, at and one above a multiple of the kernel's frames per workgroup, rows 1 .. 3 (the flat index crosses the row
    seams inside a workgroup), hops of 1 (len < win_len: every frame is partly zeros), win_len / 4, win_len and win_len + 3; the fused
    bounds 64 and 2048, lengths inside, and 32 and 4096 just outside (composed on every context)."""
    n_fft = win_len // 2
    filters = 26 if n_fft >= 128 else 8
    bins = _ref_bins(16000, n_fft, filters)
    tile = XPB.get(win_len, 4)
    mult = tile if tile >= 8 else 2 * tile
    case = 0
    for hop in (1, win_len // 4, win_len, win_len + 3):
        for frames in (mult - 1, mult, mult + 1):
            rows = 1 + case % 3
            case += 1
            length = frames * hop - hop // 2
            assert -(-length // hop) == frames
            x = fo.signal(seeded(41000 + win_len + case), rows, length)
            _check_all(ctxs, oracle, x, win_len, hop, frames, bins, f"win_len={win_len} hop={hop} rows={rows} frames={frames}", counts=[13 if filters > 13 else 5])


@pytest.mark.parametrize("win_len,hop,length", [(256, 64, 1000), (1024, 256, 700), (64, 64, 10)])
def test_more_frames_than_the_signal_fills(ctxs, oracle, win_len, hop, length):
    """frames two more than ceil(len / hop): the extra frames are silence (+0 energies, the MFCC of logf(1e-12f) rows), and a row shorter
    than the window."""
    frames = -(-length // hop) + 2
    bins = _ref_bins(16000, win_len // 2, 8)
    x = fo.signal(seeded(42000 + win_len), 3, length)
    want_e, want_c = _check_all(ctxs, oracle, x, win_len, hop, frames, bins, f"win_len={win_len} frames={frames}")
    assert bits_equal(want_e[:, -2:], np.zeros((3, 2, 8), F)), "the oracle's silence"
    quiet = mo.mfcc(np.zeros((1, 0), F), [0] * 10, 8)[0]
    assert bits_equal(want_c[0, -1], quiet) and bits_equal(want_c[2, -2], quiet)


@pytest.mark.parametrize("rate,filters", [(16000, 26), (16000, 40), (22050, 80), (22050, 128)])
def test_reference_shaped_edges(ctxs, oracle, rate, filters):
    """win_len 512: four frames per workgroup, 3 rows x 9 frames; num_coeffs 1, 13 and num_mel."""
    win_len, hop, frames, rows = 512, 160, 9, 3
    bins = _ref_bins(rate, win_len // 2, filters)
    assert bins == mo.ref_bins(rate, win_len // 2, filters)
    x = fo.signal(seeded(43000 + filters), rows, frames * hop - 7)
    want_e, _ = _check_all(ctxs, oracle, x, win_len, hop, frames, bins, f"({rate}, {filters})")
    assert np.isnan(want_e[1]).any() and np.isnan(want_e[2]).any() and not np.isnan(want_e[0, 0]).any(), "inf and NaN poison the frames that cover them"


TOP = mo.U64_MAX
HAND_MADE = [
    ("all edges equal", [5] * 6),
    ("dead filters between two live ones", [0, 4, 8, 8, 12, 16]),
    ("empty rise, non-empty fall", [3, 3, 9, 14, 20]),
    ("a filter per bin", list(range(0, 66))),
    ("one filter over the whole row", [0, 32, 64]),
    ("edges beyond n_fft", [0, 10, 30, 70, 90]),
    ("every edge beyond n_fft", [70, 80, 90, 100]),
    ("a saturated last edge", [0, 10, 30, TOP]),
]


@pytest.mark.parametrize("name,bins", HAND_MADE, ids=[h[0] for h in HAND_MADE])
def test_hand_made_edges(ctxs, oracle, name, bins):
    win_len, hop, frames, rows = 128, 32, 17, 2
    x = fo.signal(seeded(44000 + len(bins)), rows, frames * hop - 3)
    want_e, _ = _check_all(ctxs, oracle, x, win_len, hop, frames, bins, name)
    if not any(mo.live(bins)) or bins[0] >= 64:
        assert bits_equal(want_e, np.zeros(want_e.shape, F)), "no live filter inside the row: +0 energies"


@pytest.mark.parametrize("num_mel", [1, 127, 128, 129])
def test_fused_bound_on_the_filters(ctxs, oracle, num_mel):
    """One below, at and one above the fused kernel's bound on num_mel (129 runs composed on every context), and a single filter."""
    win_len, hop, frames = 512, 128, 5
    bins = [(i * 256) // (num_mel + 1) for i in range(num_mel + 2)]
    x = fo.signal(seeded(45000 + num_mel), 2, frames * hop, special=False)
    _check_all(ctxs, oracle, x, win_len, hop, frames, bins, f"num_mel={num_mel}")


# dispatch() (host_common.hip.h) on a 256-CU part: the persistent kernels start at CUs x k transforms (tests/test_gpu_stft_rows.py)
THRESH = {6: 256 * 512, 7: 256 * 256, 8: 256 * 128, 9: 256 * 64, 10: 256 * 32, 11: 256 * 16, 12: 256 * 4, 13: 256 * 4}
ROUTES = [(L, 129, 41) for L in (1, 2, 3, 4, 5)]                      # fft_small_kernel: several workgroups, a ragged last one
ROUTES += [(L, 12, THRESH[L] // 12 + 1) for L in (6, 7, 8)]           # groups of 2 / 4 frames inside a row: the persistent group kernels
ROUTES += [(L, 5, THRESH[L] // 5 + 1) for L in (9, 10, 11, 12, 13)]   # at or above the threshold, five frames per row
ROUTES += [(13, 5, 3), (14, 5, 7), (14, 4, 3)]                        # the generic kernel at 8192 and 16384


@pytest.mark.parametrize("L,frames,rows", ROUTES, ids=lambda v: str(v))
def test_composed_route_on_every_magnitudes_kernel(composed32, oracle, L, frames, rows):
    """The composed route's magnitudes run the rows policy without a maximum (StftMagRowsNoMaxIO) through dispatch(): every small,
    generic and persistent kernel it instantiates, totals made of many rows so that every kernel walks across many seams."""
    n = 1 << L
    hop = max(1, n // 4)
    length = frames * hop - min(3, hop - 1) if hop > 1 else frames
    x = (seeded(52000 + 100 * L + frames).uniform(-1, 1, (rows, length)) * (10.0 ** (np.arange(rows) % 7 - 3))[:, None]).astype(F)
    x[rows // 2] = 0.0
    x[min(rows - 1, rows // 2 + 1), length // 2] = np.nan
    bins = [(i * (n // 2)) // 5 for i in range(6)]
    _check_all([("set_frontend_fused(0)", composed32)], oracle, x, n, hop, frames, bins, f"n {n} rows {rows} x frames {frames}", counts=[3])


def test_window_32_on_the_generic_kernel(monkeypatch, oracle):
    """KOFFT_HIP_SMALL32=0 in a context of the test's own: win_len 32 on fft_wg_kernel instead of one thread per transform."""
    import kofft_amd

    monkeypatch.setenv("KOFFT_HIP_SMALL32", "0")
    f = kofft_amd.HipFftImpl(F)
    try:
        f.set_frontend_fused(0)
        x = fo.signal(seeded(52900), 3, 17 * 8 - 3)
        _check_all([("KOFFT_HIP_SMALL32=0", f)], oracle, x, 32, 8, 17, [0, 3, 7, 12, 16], "win_len=32", counts=[2])
    finally:
        f.close()


@pytest.mark.parametrize("win_len", [256, 400])
def test_a_callers_window(ctxs, oracle, win_len):
    """Hamming from kofft_hip_window_f32; 400 is a Bluestein length: composed on every context."""
    from kofft_amd import window

    win = window.hamming(win_len)
    hop, frames, rows = win_len // 4, 18, 2
    bins = _ref_bins(16000, win_len // 2, 26)
    x = fo.signal(seeded(46000 + win_len), rows, frames * hop - 1)
    _check_all(ctxs, oracle, x, win_len, hop, frames, bins, f"hamming({win_len})", window=win, counts=[13])
    # and hann through the argument is hann through the null pointer
    from kofft_amd import hann

    f = ctxs[2][1]
    a = f.stft_mfcc_rows(x, win_len, hop, bins, 13, hann(win_len), frames)
    b = f.stft_mfcc_rows(x, win_len, hop, bins, 13, None, frames)
    assert_rows_equal(a.reshape(-1, 13), b.reshape(-1, 13), "hann given / hann by default", nan_safe=True)


def test_one_sample_window(ctxs):
    """win_len == 1: n_fft == 0, +0 energies and the MFCCs of logf(1e-12f) rows."""
    x = fo.signal(seeded(46500), 2, 9, special=False)
    bins = [0, 1, 2, 3, 4]
    quiet = mo.mfcc(np.zeros((1, 0), F), bins, 3)[0]
    for name, f in ctxs:
        e = f.stft_mel_rows(x, 1, 2, bins)
        assert e.shape == (2, 5, 3) and bits_equal(e, np.zeros((2, 5, 3), F)), name
        c = f.stft_mfcc_rows(x, 1, 2, bins, 3)
        assert bits_equal(c, np.broadcast_to(quiet, (2, 5, 3))), name


def _dev_call(f, kind, d_sig, rows, length, stride, d_win, win_len, hop, frames, bins, d_out, nc=0):
    b = np.ascontiguousarray(bins, np.uint64)
    vp = lambda p: None if not p else C.c_void_p(int(p))
    args = [f._ctx, vp(d_sig), rows, length, stride, vp(d_win), win_len, hop, frames, C.c_void_p(b.ctypes.data), b.size - 2]
    if kind == "mel":
        return f._lib.kofft_hip_dev_stft_mel_f32(*args, vp(d_out))
    return f._lib.kofft_hip_dev_stft_mfcc_f32(*args, nc, vp(d_out))


@pytest.mark.parametrize("win_len,hop", [(128, 32), (1024, 256), (96, 40)])
def test_device_forms_with_a_gap_between_the_rows(ctxs, oracle, win_len, hop):
    """Device pointers: the signal 4 bytes past a 16-byte boundary, row_stride > len with NaN in the gaps (a frame at the end of a row
    reads +0, never the gap or the head of the next row), outputs pre-filled with NaN."""
    import torch

    rows, frames, num_mel, nc = 3, 19, 8, 5
    length, stride = frames * hop - 5, frames * hop + 11
    bins = _ref_bins(16000, win_len // 2, num_mel)
    x = fo.signal(seeded(47000 + win_len), rows, length)
    want_e, want_c = fo.expected(oracle, x, win_len, hop, frames, bins)
    padded = np.full((rows, stride), np.nan, F)
    padded[:, :length] = x
    d = torch.full((rows * stride + 8,), float("nan"), device="cuda")
    d[1:1 + rows * stride] = torch.from_numpy(padded.reshape(-1)).cuda()
    torch.cuda.synchronize()
    for name, f in ctxs:
        e = torch.full((rows * frames, num_mel), float("nan"), device="cuda")
        c = torch.full((rows * frames, nc), float("nan"), device="cuda")
        torch.cuda.synchronize()
        assert _dev_call(f, "mel", d.data_ptr() + 4, rows, length, stride, 0, win_len, hop, frames, bins, e.data_ptr()) == 0
        assert _dev_call(f, "mfcc", d.data_ptr() + 4, rows, length, stride, 0, win_len, hop, frames, bins, c.data_ptr(), nc) == 0
        f.synchronize()
        assert_rows_equal(e.cpu().numpy(), want_e.reshape(-1, num_mel), f"dev win_len={win_len}: energies, {name}", nan_safe=True)
        assert_rows_equal(c.cpu().numpy(), np.ascontiguousarray(want_c[:, :, :nc]).reshape(-1, nc), f"dev win_len={win_len}: coefficients, {name}", nan_safe=True)


def test_equals_the_two_call_chain_byte_for_byte(ctxs, oracle):
    """The shape of tests/test_gpu_mfcc.py's chain test (3 x 2048, window 256, hop 64): the new device call against
    stft_magnitudes_rows_dev -> mfcc_dev on the same context, byte for byte, and both against the oracle."""
    import torch

    rows, length, win_len, hop = 3, 2048, 256, 64
    frames, n_fft = length // hop, win_len // 2
    x = seeded(36000).uniform(-1, 1, (rows, length)).astype(F)
    bins = _ref_bins(16000, n_fft, 26)
    _, want_c = fo.expected(oracle, x, win_len, hop, frames, bins)
    want = np.ascontiguousarray(want_c[:, :, :13]).reshape(-1, 13)
    d_sig = torch.from_numpy(x).cuda()
    for name, f in ctxs:
        d_mags = torch.full((rows, frames, n_fft), float("nan"), device="cuda")
        d_max = torch.full((rows,), float("nan"), device="cuda")
        chain = torch.full((rows * frames, 13), float("nan"), device="cuda")
        one = torch.full((rows * frames, 13), float("nan"), device="cuda")
        torch.cuda.synchronize()
        f.stft_magnitudes_rows_dev(d_sig.data_ptr(), rows, length, length, win_len, hop, d_mags.data_ptr(), frames, d_max.data_ptr())
        f.mfcc_dev(d_mags.data_ptr(), chain.data_ptr(), n_fft, rows * frames, bins, 13)
        f.stft_mfcc_rows_dev(d_sig.data_ptr(), rows, length, length, 0, win_len, hop, frames, bins, 13, one.data_ptr())
        f.synchronize()
        assert one.cpu().numpy().tobytes() == chain.cpu().numpy().tobytes(), name
        assert_rows_equal(one.cpu().numpy(), want, f"one call, {name}", nan_safe=True)


def test_overlap_is_refused_then_one_valid_call(fft32, oracle):
    import torch

    rows, length, win_len, hop, frames = 2, 640, 128, 64, 10
    bins = [0, 8, 16, 24, 64]
    x = fo.signal(seeded(48000), rows, length, special=False)
    d = torch.from_numpy(x).cuda()
    w = torch.from_numpy(np.hamming(win_len).astype(F)).cuda()
    out = torch.full((rows * frames, 3), float("nan"), device="cuda")
    torch.cuda.synchronize()
    sig, end = d.data_ptr(), d.data_ptr() + 4 * rows * length
    for o in (sig, sig + 4 * 100, end - 4):                      # the output inside the signal: its start, its middle, its last float
        assert _dev_call(fft32, "mel", sig, rows, length, length, w.data_ptr(), win_len, hop, frames, bins, o) == 6
        assert _dev_call(fft32, "mfcc", sig, rows, length, length, 0, win_len, hop, frames, bins, o, 2) == 6
    assert _dev_call(fft32, "mel", sig, rows, length, length, w.data_ptr(), win_len, hop, frames, bins, w.data_ptr() + 4 * 127) == 6
    assert _dev_call(fft32, "mfcc", sig, rows, length, length, w.data_ptr(), win_len, hop, frames, bins, w.data_ptr() - 4 * 30, 2) == 6
    assert fft32._lib.kofft_hip_set_frontend_fused(fft32._ctx, 3) == 6 and fft32._lib.kofft_hip_set_frontend_fused(fft32._ctx, -1) == 6
    # edge sizes: nothing written
    assert _dev_call(fft32, "mel", sig, rows, length, length, 0, win_len, hop, frames, [0, 5], out.data_ptr()) == 0        # num_mel == 0
    assert _dev_call(fft32, "mfcc", sig, rows, length, length, 0, win_len, hop, frames, bins, out.data_ptr(), 0) == 0     # num_coeffs == 0
    assert _dev_call(fft32, "mfcc", 0, 0, length, length, 0, win_len, hop, frames, bins, 0, 9) == 0                       # rows == 0
    fft32.synchronize()
    assert np.isnan(out.cpu().numpy()).all() and bits_equal(d.cpu().numpy(), x), "the refused and the empty calls touched nothing"
    assert _dev_call(fft32, "mel", sig, rows, length, length, w.data_ptr(), win_len, hop, frames, bins, out.data_ptr()) == 0
    fft32.synchronize()
    want_e, _ = fo.expected(oracle, x, win_len, hop, frames, bins, np.hamming(win_len).astype(F))
    assert_rows_equal(out.cpu().numpy(), want_e.reshape(-1, 3), "one valid call after the refusals", nan_safe=True)


def test_context_lifecycle_and_streams(oracle):
    """A second context, kofft_hip_release_scratch between calls, the three modes on one context, and the device form from another
    stream (the Hann table and the plan cached on the context's own stream, a new plan uploaded on the other)."""
    import torch

    import kofft_amd

    rows, win_len, hop, frames = 2, 256, 100, 11
    x = fo.signal(seeded(49000), rows, frames * hop - 9)
    length = x.shape[1]
    sets = [_ref_bins(16000, 128, 13), [0, 20, 40, 90, 128, 200]]
    want = [fo.expected(oracle, x, win_len, hop, frames, b)[1] for b in sets]
    c1, c2 = kofft_amd.HipFftImpl(F), kofft_amd.HipFftImpl(F)
    try:
        for mode in (2, 0, 1, 2):
            c1.set_frontend_fused(mode)
            for j in (0, 1):
                nc = len(sets[j]) - 2
                assert_rows_equal(c1.stft_mfcc_rows(x, win_len, hop, sets[j], nc).reshape(-1, nc), want[j].reshape(-1, nc), f"c1 mode {mode} set {j}", nan_safe=True)
            c1.release_scratch()
        c2.set_frontend_fused(0)
        assert_rows_equal(c2.stft_mfcc_rows(x, win_len, hop, sets[1], 2).reshape(-1, 2), np.ascontiguousarray(want[1][:, :, :2]).reshape(-1, 2), "c2", nan_safe=True)
        s = torch.cuda.Stream()
        d_x = torch.from_numpy(x).cuda()
        for mode in (2, 0):
            c1.set_frontend_fused(mode)
            o_a = torch.full((rows * frames, 3), float("nan"), device="cuda")
            o_b = torch.full((rows * frames, 2), float("nan"), device="cuda")
            torch.cuda.synchronize()
            c1.set_stream(s.cuda_stream)
            c1.stft_mfcc_rows_dev(d_x.data_ptr(), rows, length, length, 0, win_len, hop, frames, sets[0], 3, o_a.data_ptr())
            c1.stft_mfcc_rows_dev(d_x.data_ptr(), rows, length, length, 0, win_len, hop, frames, [0, 64, 100, 128], 2, o_b.data_ptr())
            c1.synchronize()
            c1.set_stream(0)
            assert_rows_equal(o_a.cpu().numpy(), np.ascontiguousarray(want[0][:, :, :3]).reshape(-1, 3), f"another stream, mode {mode}", nan_safe=True)
            wb = fo.expected(oracle, x, win_len, hop, frames, [0, 64, 100, 128])[1]
            assert_rows_equal(o_b.cpu().numpy(), wb.reshape(-1, 2), f"a new plan on another stream, mode {mode}", nan_safe=True)
    finally:
        c1.close()
        c2.close()


@pytest.fixture(scope="module")
def seam_case(oracle):
    """The inputs and the expected values of test_chunk_seams_inside_a_row, computed once for both modes."""
    from kofft_amd import window

    x = fo.signal(seeded(50000), 3, 600 * 256 - 100)
    bins = _ref_bins(16000, 512, 40)
    want_e, want_c = fo.expected(oracle, x, 1024, 256, 600, bins)
    xs = np.ascontiguousarray(x[:, :50000])
    b400 = _ref_bins(16000, 200, 26)
    we, _ = fo.expected(oracle, xs, 400, 150, 334, b400, window.hamming(400))
    return x, bins, want_e, want_c, xs, b400, we


@pytest.mark.parametrize("mode", [0, 1])
def test_chunk_seams_inside_a_row(monkeypatch, seam_case, mode):
    """KOFFT_HIP_SCRATCH_CHUNK_MB=1 around the creation of a context of the test's own: 3 rows x 600 frames of 1024 are 1800 frames of
    2 KiB of magnitudes, 512 per pass -- seams inside rows 0, 1 and 2, a chunk that holds the tail of one row and the head of the next."""
    import kofft_amd

    win_len, hop = 1024, 256
    assert [min(512, 1800 - t) for t in range(0, 1800, 512)] == [512, 512, 512, 264] and (1 << 20) // (4 * 512) == 512
    x, bins, want_e, want_c, xs, b400, we = seam_case
    monkeypatch.setenv(KNOB, "1")
    f = kofft_amd.HipFftImpl(F)
    try:
        f.set_frontend_fused(mode)
        got = f.stft_mfcc_rows(x, win_len, hop, bins, 13)
        assert_rows_equal(got.reshape(-1, 13), np.ascontiguousarray(want_c[:, :, :13]).reshape(-1, 13), f"mode {mode}: coefficients across the seams", nan_safe=True)
        got = f.stft_mel_rows(x, win_len, hop, bins)
        assert_rows_equal(got.reshape(-1, 40), want_e.reshape(-1, 40), f"mode {mode}: energies across the seams", nan_safe=True)
        # a Bluestein window: [magnitudes | composed frames] share the megabyte -- 1002 frames of 200 * 4 + 400 * 8 bytes, 262 per pass
        from kofft_amd import window

        got = f.stft_mel_rows(xs, 400, 150, b400, window.hamming(400))
        assert_rows_equal(got.reshape(-1, 26), we.reshape(-1, 26), f"mode {mode}: win_len 400 across the seams", nan_safe=True)
    finally:
        f.close()


# (win_len, hop, rows, frames per row, filters, the scratch bytes of a frame, the one chunk with all three kinds of rectangle)
THREE_KINDS = [(64, 4, 7, 3000, 8, 32 * 4, (8192, 8192)),                  # the magnitudes kernels: [magnitudes]
               (1000, 300, 7, 40, 20, 500 * 4 + 1000 * 8, (104, 104))]      # composed: [magnitudes | composed frames]


@pytest.mark.parametrize("win_len,hop,rows,frames,filters,frame_bytes,chunk", THREE_KINDS, ids=["kernels-64", "composed-1000"])
def test_a_chunk_with_the_tail_of_a_row_whole_rows_and_the_head_of_a_row(monkeypatch, fft32, oracle, win_len, hop, rows, frames, filters,
                                                                        frame_bytes, chunk):
    """KOFFT_HIP_SCRATCH_CHUNK_MB=1: 7 rows whose second chunk holds the tail of row 2, rows 3 and 4 and the head of row 5 -- the
    producer's magnitudes per rectangle (808 + 2 x 3000 + 1384 frames of 64) and its composed magnitudes (16 + 2 x 40 + 8 frames of
    1000).  Energies and coefficients against the oracle and against the same call on a default context, bit for bit."""
    import kofft_amd
    from test_gpu_scratch_seams import chunk_kinds, three_kind_chunks

    assert three_kind_chunks(1, frame_bytes, rows, frames) == [chunk]
    assert chunk_kinds(*chunk, frames) == ((808, 6000, 1384) if win_len == 64 else (16, 80, 8))
    x = fo.signal(seeded(51000 + win_len), rows, frames * hop - hop // 2)
    bins = _ref_bins(16000, win_len // 2, filters)
    want_e, want_c = fo.expected(oracle, x, win_len, hop, frames, bins)
    nc = min(13, filters)
    monkeypatch.setenv(KNOB, "1")
    f = kofft_amd.HipFftImpl(F)
    try:
        f.set_frontend_fused(0)
        got_e, got_c = f.stft_mel_rows(x, win_len, hop, bins), f.stft_mfcc_rows(x, win_len, hop, bins, nc)
        assert_rows_equal(got_e.reshape(-1, filters), want_e.reshape(-1, filters), f"win_len {win_len}: energies", nan_safe=True)
        assert_rows_equal(got_c.reshape(-1, nc), np.ascontiguousarray(want_c[:, :, :nc]).reshape(-1, nc), f"win_len {win_len}: coefficients",
                          nan_safe=True)
        assert bits_equal(got_e, fft32.stft_mel_rows(x, win_len, hop, bins)), "energies differ from the default context's"
        assert bits_equal(got_c, fft32.stft_mfcc_rows(x, win_len, hop, bins, nc)), "coefficients differ from the default context's"
    finally:
        f.close()
