"""cepstrum::mel_filterbank / mfcc on the device with the filter edges as an input, every row bit for bit against tests/mel_oracle.py
(NaNs by position: the host and the device produce different default NaNs).  Every case runs the MFCC on the default context (the
fused kernel up to 80 filters and 16 coefficients, composed beyond), on the composed route (set_mfcc_fused(0)) and on the fused
kernel wherever it fits (set_mfcc_fused(2)), and the filterbank alone against the oracle's energies.

Shapes: mel_kernel walks k in tiles of 32 and owns 64 rows per workgroup; its results leave 32 per row at a time; rows of n_fft % 4 == 0
values on a 16-byte aligned input load 16 bytes per lane (VEC), everything else 4; the fused kernel takes num_mel <= 128 and runs the
DCT eight outputs at a time.  Kernel instances and the tests that launch them are listed in DESIGN.md 5.21."""
import ctypes as C

import numpy as np
import pytest

import mel_oracle as mo
from conftest import bits_equal, seeded
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32
ROWS = [1, 2, 63, 64, 65, 129, 257]


@pytest.fixture(scope="module")
def composed32():
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_mfcc_fused(False)
    yield f
    f.close()


@pytest.fixture(scope="module")
def forced32():
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_mfcc_fused(2)
    yield f
    f.close()


def _rows(n, rows, seed):
    """|N(0, 1)| rows; then, where the batch and the row have room: row 1 all +0, row 2 with a -0, row 3 with a subnormal, row 4 with
    negative values (the log of a negative energy is NaN), row 5 with inf and NaN."""
    x = np.abs(seeded(seed).standard_normal((rows, n))).astype(F)
    if n == 0:
        return x
    if rows > 1:
        x[1] = 0.0
    if rows > 2:
        x[2, n // 2] = -0.0
    if rows > 3:
        x[3, n // 3] = 1e-41
        x[3, 0] = 1e-45
    if rows > 4:
        x[4] = -x[4]
        x[4, 1::5] *= F(-0.25)  # (mostly negative: every filter of more than a few values sums below zero)
    if rows > 5:
        x[5, 0] = np.inf
        x[5, n // 2] = np.nan
        x[5, n - 1] = -np.inf
    return x


def _coeff_counts(num_mel):
    return sorted({min(1, num_mel), min(13, num_mel), num_mel})


def _check_all(fft32, composed32, forced32, x, bins, what, counts=None):
    """Default, composed, fused-wherever-it-fits and filterbank-only on the host forms against the oracle, every row."""
    num_mel = len(bins) - 2
    want_e = mo.energies(x, bins)
    want_c = mo.mfcc(x, bins, num_mel)
    got_e = fft32.mel_filterbank_batch(x, bins)
    assert_rows_equal(got_e, want_e, what + ": energies", nan_safe=True)
    assert bits_equal(got_e, fft32.mel_filterbank_batch(x, bins)), what + ": two runs differ"
    for nc in counts or _coeff_counts(num_mel):
        want = np.ascontiguousarray(want_c[:, :nc])
        got = fft32.mfcc_batch(x, bins, nc)
        assert_rows_equal(got, want, f"{what} nc={nc}: default", nan_safe=True)
        assert_rows_equal(composed32.mfcc_batch(x, bins, nc), got, f"{what} nc={nc}: set_mfcc_fused(0)", nan_safe=True)
        assert_rows_equal(forced32.mfcc_batch(x, bins, nc), got, f"{what} nc={nc}: set_mfcc_fused(2)", nan_safe=True)
    return got_e, want_c


@pytest.mark.parametrize("setting", mo.SETTINGS)
def test_reference_shaped_edges(fft32, composed32, forced32, setting):
    from kofft_amd import mfcc

    rate, n_fft, filters = setting
    bins = [int(b) for b in mfcc.mel_bins(float(rate), n_fft, filters)]
    assert bins == mo.ref_bins(rate, n_fft, filters)
    row_counts = ROWS if n_fft in (32, 256) else ([130] if n_fft == 1024 else [65])
    x_all = _rows(n_fft, max(row_counts), 31000 + n_fft + filters)
    want_e = mo.energies(x_all, bins)  # once per setting: a row's result does not depend on the batch
    want_c = mo.mfcc(x_all, bins, filters)
    for rows in row_counts:
        x = np.ascontiguousarray(x_all[:rows])
        what = f"{setting} rows={rows}"
        assert_rows_equal(fft32.mel_filterbank_batch(x, bins), want_e[:rows], what + ": energies", nan_safe=True)
        for nc in _coeff_counts(filters):
            want = np.ascontiguousarray(want_c[:rows, :nc])
            got = fft32.mfcc_batch(x, bins, nc)
            assert_rows_equal(got, want, f"{what} nc={nc}: default", nan_safe=True)
            assert_rows_equal(composed32.mfcc_batch(x, bins, nc), got, f"{what} nc={nc}: set_mfcc_fused(0)", nan_safe=True)
            assert_rows_equal(forced32.mfcc_batch(x, bins, nc), got, f"{what} nc={nc}: set_mfcc_fused(2)", nan_safe=True)
    if any(mo.live(bins)) and max(row_counts) > 5:
        assert np.isnan(want_c[4]).any(), "the log of a negative energy is NaN, and the DCT spreads it"
        assert bits_equal(want_e[1], np.zeros(filters, F)), "a row of +0 gives +0 energies"


TOP = mo.U64_MAX
HAND_MADE = [
    ("all edges equal", 16, [5] * 6),
    ("dead filters between two live ones", 24, [0, 4, 8, 8, 12, 16]),
    ("empty rise, non-empty fall", 24, [3, 3, 9, 14, 20]),
    ("edges beyond the row", 40, [0, 10, 30, 50, 70]),
    ("a saturated last edge", 40, [0, 10, 30, TOP]),
    ("every edge beyond the row", 16, [50, 60, 70, 80]),
    ("denominators beyond 2^24", 40, [0, 10, (1 << 24) + 1, (1 << 40) + 3, TOP]),
    ("one filter over the row, n=64", 64, [0, 32, 64]),
    ("one filter over the row, n=33", 33, [0, 16, 33]),
    ("one filter over the row, n=7", 7, [0, 3, 7]),
    ("one filter over the row, n=1", 1, [0, 0, 1]),
    ("one live filter on one value", 1, [0, 1, 2]),
    ("edges on and around every tile seam", 200, [0, 31, 32, 33, 63, 64, 65, 95, 96, 97, 128, 160, 192, 200]),
    ("a filter per value", 70, list(range(0, 71))),
    ("first edge inside a later tile", 130, [70, 90, 97, 130]),
    ("n=7, generic", 7, [0, 1, 2, 4, 7]),
    ("n=33, generic", 33, [1, 5, 9, 20, 33, 40]),
    ("no rows of data: n_fft = 0", 0, [0, 2, 4, 6]),
]


@pytest.mark.parametrize("name,n_fft,bins", HAND_MADE, ids=[h[0] for h in HAND_MADE])
def test_hand_made_edges(fft32, composed32, forced32, name, n_fft, bins):
    x = _rows(n_fft, 70, 32000 + n_fft + len(bins))
    got_e, want_c = _check_all(fft32, composed32, forced32, x, bins, name)
    if not any(mo.live(bins)) or n_fft == 0:
        assert bits_equal(got_e, np.zeros(got_e.shape, F)), "no live filter, or no data: +0 energies"
        assert bits_equal(want_c[0], mo.mfcc(np.zeros((1, 0), F), [0] * len(bins), len(bins) - 2)[0]), "the MFCC of logf(1e-12f) rows"


@pytest.mark.parametrize("num_mel", [127, 128, 129])
def test_fused_bound(fft32, composed32, forced32, num_mel):
    """One below, at and one above the fused kernel's bound on num_mel, n_fft = 1024, evenly spaced edges: 129 filters run composed on
    every context; 13, 16 and 17 coefficients straddle the default's bound on num_coeffs."""
    n_fft = 1024
    bins = [(i * n_fft) // (num_mel + 1) for i in range(num_mel + 2)]
    x = _rows(n_fft, 66, 33000 + num_mel)
    _check_all(fft32, composed32, forced32, x, bins, f"num_mel={num_mel}", counts=[13, 16, 17, num_mel])


@pytest.mark.parametrize("num_mel", [80, 81])
def test_default_route_bounds(fft32, composed32, forced32, num_mel):
    """Both sides of the default's bounds: 80 / 81 filters, 16 / 17 coefficients."""
    n_fft = 256
    bins = [(i * 300) // (num_mel + 1) for i in range(num_mel + 2)]
    x = _rows(n_fft, 66, 33200 + num_mel)
    _check_all(fft32, composed32, forced32, x, bins, f"num_mel={num_mel}", counts=[16, 17])


def test_many_filters_composed(fft32):
    """Far above the bound: 300 filters over 700 values (the filterbank's output tile flushes ten times per row, the last one partial)."""
    bins = [(i * 700) // 301 for i in range(302)]
    x = _rows(700, 65, 33500)
    want = mo.mfcc(x, bins, 300)
    assert_rows_equal(fft32.mfcc_batch(x, bins, 300), want, "300 filters", nan_safe=True)
    assert_rows_equal(fft32.mfcc_batch(x, bins, 40), np.ascontiguousarray(want[:, :40]), "300 filters, 40 coefficients", nan_safe=True)
    assert_rows_equal(fft32.mel_filterbank_batch(x, bins), mo.energies(x, bins), "300 filters: energies", nan_safe=True)


def _dev_call(f, kind, d_in, d_out, n_fft, rows, bins, nc=0):
    b = np.ascontiguousarray(bins, np.uint64)
    pb = C.c_void_p(b.ctypes.data)
    p_in, p_out = (None if p is None else C.c_void_p(int(p)) for p in (d_in, d_out))
    if kind == "mel":
        return f._lib.kofft_hip_dev_mel_filterbank_f32(f._ctx, p_in, p_out, n_fft, rows, pb, b.size - 2)
    return f._lib.kofft_hip_dev_mfcc_f32(f._ctx, p_in, p_out, n_fft, rows, pb, b.size - 2, nc)


@pytest.mark.parametrize("n_fft,off", [(64, 1), (64, 0), (33, 0), (33, 1), (7, 1), (1, 1)])
def test_device_form_and_misaligned_input(fft32, composed32, forced32, n_fft, off):
    """d_mags offset by one float (4-byte aligned only) and odd rows: the 4-byte loads; (64, 0): the 16-byte loads."""
    import torch

    rows = 70
    bins = sorted({0, n_fft // 3, n_fft // 2, n_fft, n_fft + 5}) if n_fft > 1 else [0, 1, 2]
    num_mel = len(bins) - 2
    x = _rows(n_fft, rows, 34000 + n_fft)
    d = torch.zeros(rows * n_fft + 4, device="cuda")
    d[off:off + rows * n_fft] = torch.from_numpy(x.reshape(-1)).cuda()
    want_e, want_c = mo.energies(x, bins), mo.mfcc(x, bins, num_mel)
    for f in (fft32, composed32, forced32):
        e = torch.full((rows, num_mel), float("nan"), device="cuda")
        c = torch.full((rows, num_mel), float("nan"), device="cuda")
        assert _dev_call(f, "mel", d.data_ptr() + 4 * off, e.data_ptr(), n_fft, rows, bins) == 0
        assert _dev_call(f, "mfcc", d.data_ptr() + 4 * off, c.data_ptr(), n_fft, rows, bins, num_mel) == 0
        f.synchronize()
        assert_rows_equal(e.cpu().numpy(), want_e, f"dev n_fft={n_fft} off={off}: energies", nan_safe=True)
        assert_rows_equal(c.cpu().numpy(), want_c, f"dev n_fft={n_fft} off={off}: coefficients", nan_safe=True)


def test_argument_edges_on_a_live_context(fft32):
    import torch

    d = torch.zeros(4 * 64, device="cuda")
    bins = [0, 8, 16, 24]
    # overlapping device buffers: INVALID_VALUE; adjacent is not overlap; then one valid call
    assert _dev_call(fft32, "mel", d.data_ptr(), d.data_ptr() + 4 * 8, 32, 3, bins) == 6
    assert _dev_call(fft32, "mfcc", d.data_ptr(), d.data_ptr(), 32, 3, bins, 2) == 6
    assert _dev_call(fft32, "mfcc", d.data_ptr(), d.data_ptr() + 4 * 96, 32, 3, bins, 2) == 0
    fft32.synchronize()
    # edge sizes: nothing written, no pointer read
    assert _dev_call(fft32, "mel", d.data_ptr(), d.data_ptr(), 32, 3, [0, 5]) == 0       # num_mel == 0
    assert _dev_call(fft32, "mfcc", d.data_ptr(), d.data_ptr(), 32, 3, bins, 0) == 0    # num_coeffs == 0
    assert _dev_call(fft32, "mfcc", None, None, 32, 0, bins, 9) == 0                    # rows == 0
    assert _dev_call(fft32, "mfcc", d.data_ptr(), d.data_ptr() + 512, 32, 3, bins, 3) == 6
    assert _dev_call(fft32, "mel", d.data_ptr(), d.data_ptr() + 512, 32, 3, [0, 9, 8, 24]) == 6
    assert _dev_call(fft32, "mel", None, d.data_ptr(), 32, 3, bins) == -3
    assert fft32._lib.kofft_hip_set_mfcc_fused(fft32._ctx, 3) == 6 and fft32._lib.kofft_hip_set_mfcc_fused(fft32._ctx, -1) == 6
    assert fft32.mfcc_batch(np.ones((3, 32), F), bins, 0).shape == (3, 0)
    assert fft32.mel_filterbank_batch(np.ones((3, 32), F), [0, 5]).shape == (3, 0)
    assert fft32.mfcc_batch(np.ones((0, 32), F), bins, 2).shape == (0, 2)


def test_context_lifecycle_and_streams():
    """Edge sets used alternately on one context (plan reuse), more sets than the context keeps (eviction), a second context,
    kofft_hip_release_scratch between calls, and a cached plan and a new one from another stream."""
    import torch

    import kofft_amd

    n_fft, rows = 96, 70
    x = _rows(n_fft, rows, 35000)
    sets = [[0, 10, 20, 40, 96], [0, 10, 20, 41, 96], [5, 5, 30, 60, 90, 120], [0, 48, 96], [1, 2, 3, 4, 5, 6, 7], [0, 96, 200]]
    want = [mo.mfcc(x, b, len(b) - 2) for b in sets]
    c1, c2 = kofft_amd.HipFftImpl(F), kofft_amd.HipFftImpl(F)
    try:
        for _ in range(3):
            for j in (0, 1):
                assert_rows_equal(c1.mfcc_batch(x, sets[j], len(sets[j]) - 2), want[j], f"c1 set {j}", nan_safe=True)
        for j in (2, 3, 4, 5, 0, 5, 1):  # six plans through four slots
            assert_rows_equal(c1.mfcc_batch(x, sets[j], len(sets[j]) - 2), want[j], f"c1 set {j} after eviction", nan_safe=True)
        assert_rows_equal(c2.mfcc_batch(x, sets[1], 3), want[1], "c2 set 1", nan_safe=True)
        shorter = np.ascontiguousarray(x[:, :95])  # the same edges on another n_fft are another plan
        assert_rows_equal(c1.mfcc_batch(shorter, sets[0], 3), mo.mfcc(shorter, sets[0], 3), "c1 set 0, n_fft=95", nan_safe=True)
        c1.release_scratch()
        assert_rows_equal(c1.mfcc_batch(x, sets[0], 3), want[0], "c1 after release_scratch", nan_safe=True)
        c1.set_mfcc_fused(False)
        assert_rows_equal(c1.mfcc_batch(x, sets[2], 4), want[2], "c1 composed after release_scratch", nan_safe=True)
        c1.set_mfcc_fused(True)
        # device form: the plan of set 0 was uploaded on the context's own stream, the plan of set 3 is uploaded on s
        s = torch.cuda.Stream()
        d_x = torch.from_numpy(x).cuda()
        o_a = torch.full((rows, 3), float("nan"), device="cuda")
        o_b = torch.full((rows, 1), float("nan"), device="cuda")
        torch.cuda.synchronize()
        c1.set_stream(s.cuda_stream)
        c1.mfcc_dev(d_x.data_ptr(), o_a.data_ptr(), n_fft, rows, sets[0], 3)
        c1.mfcc_dev(d_x.data_ptr(), o_b.data_ptr(), n_fft, rows, sets[3], 1)
        c1.synchronize()
        c1.set_stream(0)
        assert_rows_equal(o_a.cpu().numpy(), want[0], "cached plan on another stream", nan_safe=True)
        assert_rows_equal(o_b.cpu().numpy(), want[3], "plan uploaded on another stream", nan_safe=True)
        assert_rows_equal(c1.mfcc_batch(x, sets[3], 1), want[3], "back on the own stream", nan_safe=True)
    finally:
        c1.close()
        c2.close()


def test_chain_from_stft_magnitudes_without_leaving_the_device(fft32, composed32, oracle):
    """stft_magnitudes_rows_dev -> mfcc_dev on 3 signals x 2048 samples, window 256, hop 64: the two oracles composed."""
    import torch

    from kofft_amd import mfcc

    rows, length, win_len, hop = 3, 2048, 256, 64
    x = seeded(36000).uniform(-1, 1, (rows, length)).astype(F)
    ref = [oracle.stft_magnitudes(r, win_len, hop) for r in x]
    mags = np.stack([m for m, _ in ref])
    frames, n_fft = mags.shape[1], win_len // 2
    bins = [int(b) for b in mfcc.mel_bins(16000.0, n_fft, 26)]
    want = mo.mfcc(mags.reshape(rows * frames, n_fft), bins, 13)
    d_sig = torch.from_numpy(x).cuda()
    for f in (fft32, composed32):
        d_mags = torch.full((rows, frames, n_fft), float("nan"), device="cuda")
        d_max = torch.full((rows,), float("nan"), device="cuda")
        d_out = torch.full((rows * frames, 13), float("nan"), device="cuda")
        f.stft_magnitudes_rows_dev(d_sig.data_ptr(), rows, length, length, win_len, hop, d_mags.data_ptr(), frames, d_max.data_ptr())
        f.mfcc_dev(d_mags.data_ptr(), d_out.data_ptr(), n_fft, rows * frames, bins, 13)
        f.synchronize()
        assert_rows_equal(d_mags.cpu().numpy().reshape(rows * frames, n_fft), mags.reshape(rows * frames, n_fft), "the magnitudes")
        assert_rows_equal(d_out.cpu().numpy(), want, "stft_magnitudes_rows_dev -> mfcc_dev", nan_safe=True)


def test_the_references_own_tests_on_the_device(fft32):
    """cepstrum.rs:121-148 through kofft_amd.mfcc, and the module's ragged lists."""
    import kofft_amd
    from kofft_amd import mfcc

    frames = [np.full(32, 1.0, F), np.full(32, 0.5, F)]
    got = mfcc.mfcc_batch(frames, 16000.0, 8, 4, fft=fft32)
    want = mo.mfcc(np.stack(frames), mo.ref_bins(16000, 32, 8), 4)
    assert len(got) == 2 and got[0].shape == (4,)
    assert bits_equal(np.stack(got), want)
    with pytest.raises(kofft_amd.FftError) as e:
        mfcc.mfcc(frames[0], 16000.0, 8, 20, fft=fft32)
    assert e.value.code == 6
    en = mfcc.mel_filterbank(np.ones(8, F), 8000.0, 40, fft=fft32)
    assert en.shape == (40,) and bits_equal(en, np.zeros(40, F))
    rng = seeded(37000)
    rows = [np.abs(rng.standard_normal(m)).astype(F) for m in (32, 256, 32, 64, 0, 256)]
    got = mfcc.mfcc_batch(rows, 16000.0, 8, 5)  # the module's own context
    for r, g in zip(rows, got):
        assert bits_equal(g, mo.mfcc(r[None], mo.ref_bins(16000, r.size, 8), 5)[0]), r.size
    one_sided = [0, 4, 9, 15, 22, 30, 40, 52, 64, 64]  # edges the reference cannot express, over a 64-value row
    got = mfcc.mel_filterbank(rows[3], 16000.0, 8, bins=one_sided, fft=fft32)
    assert bits_equal(got, mo.energies(rows[3][None], one_sided)[0])
