"""The polyphase filter bank of DESIGN.md 5.34 without a GPU: the oracle of tests/pfb_oracle.py against float64 direct evaluations of
both definitions, the fold on small integers, the T = 1 analysis against the oracle's STFT bit for bit, the two host helpers
(kofft_hip_pfb_taps_f32, kofft_hip_pfb_reconstruction), the round trip of the two reconstructing pairs on the oracle, the C entries'
argument checks in the header's order (a null context comes last, so none of them needs a device) and the Python module's errors, which
are raised before any context is created.

Accuracy bounds, relative L2 against float64 on uniform(-1, 1), 3 rows.  The transform bound of tests/test_mdct_cpu.py for one M-point
transform, 1e-6 + 2e-7 M, scaled by the T-term sum: each u[j] is a sum of T products (T - 1 roundings of the accumulator and T of the
products on top of the transform's own error), so the bound is T times the transform's.  M a power of two (and M = 2): that bound; it
holds with room (measured below, printed by the tests).  M = 240 takes the oracle's Bluestein arm, whose error exceeds it: BLUESTEIN
holds twice the worst measured error of the oracle over seeds 0 .. 7 per direction, T = 1 (the T-scaling then applies as above).
ROUND_TRIP: twice the worst of seeds 100 .. 104 of synthesis_ref(analysis_ref(x)) against x for the two reconstructing pairs."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits_equal, seeded
import pfb_oracle as po

F = np.float32
MS = [2, 16, 64, 240, 1024]
TS = [1, 3, 4]
# M -> (analysis, synthesis): 2 x the worst relative L2 error of the oracle at T = 1 over seeds 0 .. 7, where M is not a power of two
BLUESTEIN = {240: (2 * 3.61e-5, 2 * 3.81e-5)}
# M -> bound of the oracle's round trip, sine pair (T = 1 and the same window in block 1 of T = 3), D = M / 2: 2 x the worst of seeds 100 .. 104
ROUND_TRIP = {2: 2 * 7.27e-8, 16: 2 * 8.24e-8, 64: 2 * 4.36e-7, 240: 2 * 5.10e-5, 1024: 2 * 2.58e-5}


def bound(m: int, taps: int, which: int = 0) -> float:
    one = 1e-6 + 2e-7 * m if m & (m - 1) == 0 else BLUESTEIN[m][which]
    return taps * one


def rel(a, b) -> float:
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def sine_pair(m: int, taps: int = 1):
    """The sine window of M values for D = M / 2: alone (T = 1), or in block t = 1 of a T = 3 array of zeros."""
    w = np.sin(np.pi * (np.arange(m, dtype=np.float64) + 0.5) / m).astype(F)
    if taps == 1:
        return w
    h = np.zeros(taps * m, F)
    h[m:2 * m] = w
    return h


def analysis_f64(x, h, m, hop, lead, frames):
    """Z[k] = sum_{i < nh} h[i] x[fD + i - lead] exp(-2 pi i k i / M), all M bins, in float64"""
    rows, nx = x.shape
    nh = h.size
    xp = np.zeros((rows, lead + max(nx, frames * hop + nh)))
    xp[:, lead:lead + nx] = x
    seg = np.stack([xp[:, f * hop:f * hop + nh] for f in range(frames)], axis=1) * h.astype(np.float64)
    e = np.exp(-2j * np.pi * np.outer(np.arange(nh), np.arange(m)) / m)
    return seg @ e


def synthesis_f64(spec, g, m, hop, scale):
    rows, frames, _ = spec.shape
    nh = g.size
    r = np.fft.ifft(po.complete(spec, m).astype(np.complex128), axis=-1).real
    full = np.zeros((rows, (frames - 1) * hop + nh))
    idx = np.arange(nh)
    for f in range(frames):
        full[:, f * hop:f * hop + nh] += g.astype(np.float64) * r[:, f, idx % m]
    return full * float(F(scale))


@pytest.mark.parametrize("taps", TS)
@pytest.mark.parametrize("m", MS)
def test_oracle_against_float64(oracle, m, taps):
    rows, nh = 3, taps * m
    hop = max(m // 2, 1) + (1 if m > 2 else 0)
    nx = 3 * nh + 5
    rng = seeded(14000 + 10 * m + taps)
    x = rng.uniform(-1, 1, (rows, nx)).astype(F)
    h = rng.uniform(0.1, 1, nh).astype(F)
    for lead in sorted({0, nh - 1, max(nh - hop, 0)}):
        frames = -(-(nx + lead) // hop) + 1
        Z = po.analysis_ref(x, h, m, hop, lead, frames, m)
        err = rel(Z, analysis_f64(x, h, m, hop, lead, frames))
        print(f"M={m} T={taps} lead={lead}: analysis relative L2 error {err:.3g}, bound {bound(m, taps):.3g}")
        assert err <= bound(m, taps)
    # the synthesis of random frames, both forms of bins
    frames = 6
    forms = [m] + ([m // 2 + 1] if m % 2 == 0 and m > 2 else [])
    for bins in forms:
        S = (rng.uniform(-1, 1, (rows, frames, bins)) + 1j * rng.uniform(-1, 1, (rows, frames, bins))).astype(np.complex64)
        got = po.synthesis_ref(S, h, m, hop, 0.5)
        err = rel(got, synthesis_f64(S, h, m, hop, 0.5))
        print(f"M={m} T={taps} bins={bins}: synthesis relative L2 error {err:.3g}, bound {bound(m, taps, 1):.3g}")
        assert err <= bound(m, taps, 1)


def test_fold_on_small_integers():
    """M = 4, T = 3, D = 3, lead = 2, integer taps and samples: every product and sum is exact."""
    m, hop, lead = 4, 3, 2
    x = np.arange(1, 12, dtype=F)[None]          # 1 .. 11
    h = np.arange(1, 13, dtype=F)                # 1 .. 12
    frames = 6
    g = po.terms(x, h, hop, lead, frames)
    xp = np.concatenate([np.zeros(lead), x[0], np.zeros(40)])
    want_g = np.array([[h[i] * xp[f * hop + i] for i in range(12)] for f in range(frames)])
    assert g[0].tolist() == want_g.tolist()
    u = po.fold(g, m)
    want_u = want_g[:, 0:4] + want_g[:, 4:8] + want_g[:, 8:12]
    assert u[0].tolist() == want_u.tolist()
    # the fold is the transform's aliasing: the M-point DFT of u is the direct sum over all nh taps
    assert np.allclose(np.fft.fft(want_u, axis=-1), analysis_f64(x, h, m, hop, lead, frames)[0], atol=1e-9)
    # a frame past the end (frame 5 starts at sample 13 of 11) is exactly +0
    assert not g[0, 5].any() and not np.signbit(u[0, 5]).any()
    # a first term of -0 starts the accumulator: (-0) + (-0) stays -0 where 0 + (-0) would not
    gz = np.array([[-0.0, 1.0, -0.0, 2.0]], F)
    assert np.signbit(po.fold(gz, 2)[0, 0]) and po.fold(gz, 2)[0].tolist() == [-0.0, 3.0]


@pytest.mark.parametrize("m,hop", [(16, 16), (64, 24), (240, 100), (1024, 512)])
def test_one_tap_per_channel_is_the_stft(oracle, m, hop):
    """T = 1, lead = 0: bit for bit pyoracle.stft_mt with window h and hop D -- the frames inside the row, and the ones that reach past
    its end as well (stft() wants ceil(nx / hop) frames), since both pad with +0."""
    from oracle import pyoracle

    rng = seeded(14100 + m)
    nx = 6 * m + 7
    x = rng.uniform(-1, 1, nx).astype(F)
    h = rng.uniform(0.1, 1, m).astype(F)
    inside, frames = (nx - m) // hop + 1, -(-nx // hop)
    want = pyoracle.stft_mt(x, h, hop, frames)
    got = po.analysis_ref(x[None], h, m, hop, 0, frames, m)[0]
    want = want.reshape(frames, m)
    assert inside < frames and bits_equal(got[:inside], want[:inside])
    assert bits_equal(got, want)


@pytest.mark.parametrize("m,taps,beta", [(1, 1, 5.0), (2, 3, 0.0), (16, 4, 5.0), (64, 8, 9.0), (1024, 4, 6.5)])
def test_taps_helper(m, taps, beta):
    from kofft_amd import pfb

    got = pfb.prototype(m, taps, beta)
    nh = m * taps
    i = np.arange(nh, dtype=np.float64)
    want = np.sinc((i - (nh - 1) / 2) / m) * np.kaiser(nh, beta)
    want = want / want.sum()
    w32 = want.astype(F)
    assert got.dtype == F and got.shape == (nh,)
    assert np.all(np.abs(got.astype(np.float64) - w32.astype(np.float64)) <= np.spacing(np.abs(w32)).astype(np.float64))
    assert abs(float(got.astype(np.float64).sum()) - 1.0) <= 1e-6


def test_taps_and_reconstruction_checks():
    from kofft_amd import _lib

    lib = _lib.load()
    buf = np.zeros(8, F)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.kofft_hip_pfb_taps_f32(0, 2, 5.0, p) == 1       # EMPTY_INPUT
    assert lib.kofft_hip_pfb_taps_f32(2, 0, -1.0, None) == 1
    assert lib.kofft_hip_pfb_taps_f32(2, 2, -1.0, None) == 6   # INVALID_VALUE
    assert lib.kofft_hip_pfb_taps_f32(2, 2, float("nan"), None) == 6
    assert lib.kofft_hip_pfb_taps_f32(2, 2, 5.0, None) == -3
    c, w = C.c_double(), C.c_double()
    assert lib.kofft_hip_pfb_reconstruction(None, None, 0, 4, 0, None, None) == 1
    assert lib.kofft_hip_pfb_reconstruction(None, None, 6, 4, 0, None, None) == 6
    assert lib.kofft_hip_pfb_reconstruction(None, None, 8, 4, 0, None, None) == 5   # INVALID_HOP_SIZE
    assert lib.kofft_hip_pfb_reconstruction(None, None, 8, 4, 2, None, None) == -3
    assert lib.kofft_hip_pfb_reconstruction(p, p, 8, 4, 2, C.byref(c), C.byref(w)) == 0


@pytest.mark.parametrize("m", [2, 16, 64, 240, 1024])
def test_reconstruction_of_the_two_pairs(m):
    from kofft_amd import pfb

    for taps in (1, 3):
        h = sine_pair(m, taps)
        c, worst = pfb.reconstruction(h, h, m, m // 2)
        print(f"M={m} T={taps}: c = {c!r}, worst = {worst:.3g}")
        assert abs(c - 1.0) <= 1e-6 and worst <= 1e-6
    # a sinc x Kaiser prototype on both sides does not reconstruct
    if m >= 16:
        p = pfb.prototype(m, 4)
        c, worst = pfb.reconstruction(p, p, m, m)
        assert worst > 1e-3 * abs(c)


@pytest.mark.parametrize("m", [2, 16, 64, 240, 1024])
def test_oracle_round_trip_of_the_two_pairs(oracle, m):
    hop = m // 2
    for taps in (1, 3):
        h = sine_pair(m, taps)
        nh, lead = h.size, h.size - hop
        worst = 0.0
        for seed in range(100, 105):
            x = np.random.default_rng(seed).uniform(-1, 1, (3, 5 * m + 3)).astype(F)
            nx = x.shape[1]
            frames = -(-(nx + lead) // hop)
            Z = po.analysis_ref(x, h, m, hop, lead, frames, m // 2 + 1 if m > 2 else m)
            full = po.synthesis_ref(Z, h, m, hop, 1.0)
            worst = max(worst, rel(full[:, lead:lead + nx], x))
        print(f"M={m} T={taps}: round trip relative L2 error {worst:.3g}, bound {ROUND_TRIP[m]:.3g}")
        assert worst <= ROUND_TRIP[m]


def test_c_checks_in_header_order():
    """Each call trips one check and would trip every later one as well; the null context is the last."""
    from kofft_amd import _lib

    lib = _lib.load()
    OK, EMPTY, MISMATCH, HOP, INVALID, UNSUPPORTED, NULL = 0, 1, 3, 5, 6, -2, -3
    buf = np.zeros(64, F)
    p = C.c_void_p(buf.ctypes.data)
    big = (1 << 25) + 1  # not a power of two and above 2^25
    for fn in (lib.kofft_hip_pfb_analysis_f32, lib.kofft_hip_dev_pfb_analysis_f32):
        # (ctx, x, rows, nx, row_stride, h, nh, M, D, lead, out, frames, bins)
        assert fn(None, None, 0, 0, 0, None, 0, 0, 0, 99, None, 5, 0) == OK
        assert fn(None, None, 2, 0, 0, None, 0, 0, 0, 99, None, 0, 0) == OK
        assert fn(None, None, 2, 0, 0, None, 7, 0, 0, 99, None, 5, 0) == EMPTY        # M == 0
        assert fn(None, None, 2, 0, 0, None, 0, 4, 0, 99, None, 5, 0) == EMPTY        # nh == 0
        assert fn(None, None, 2, 0, 0, None, 7, 4, 0, 99, None, 5, 0) == INVALID      # nh % M
        assert fn(None, None, 2, 0, 0, None, 8, 4, 0, 99, None, 5, 0) == INVALID      # bins == 0
        assert fn(None, None, 2, 0, 0, None, 8, 4, 0, 99, None, 5, 5) == INVALID      # bins > M
        assert fn(None, None, 2, 0, 0, None, 2 * big, big, 0, 1 << 40, None, 5, 1) == UNSUPPORTED
        assert fn(None, None, 2, 0, 0, None, 8, 4, 0, 99, None, 5, 3) == HOP
        assert fn(None, None, 2, 0, 0, None, 8, 4, 2, 99, None, 5, 3) == EMPTY        # nx == 0
        assert fn(None, None, 2, 10, 5, None, 8, 4, 2, 8, None, 5, 3) == INVALID      # lead >= nh
        assert fn(None, None, 2, 10, 5, None, 8, 4, 2, 7, None, 5, 3) == INVALID      # row_stride < nx
        assert fn(None, None, 1, 10, 5, None, 8, 4, 2, 7, None, 1 << 61, 3) == UNSUPPORTED
        assert fn(None, None, 1, 10, 5, None, 8, 4, 1 << 61, 7, None, 16, 3) == UNSUPPORTED
        assert fn(None, None, 1, 10, 5, None, 8, 4, 2, 7, None, 5, 3) == NULL         # (rows == 1: the stride is ignored)
        assert fn(None, p, 2, 10, 10, p, 8, 4, 2, 7, p, 5, 3) == NULL
    one = C.c_float(1.0)
    for fn in (lib.kofft_hip_pfb_synthesis_f32, lib.kofft_hip_dev_pfb_synthesis_f32):
        # (ctx, spec, rows, frames, bins, g, nh, M, D, scale, out, out_first, out_len)
        assert fn(None, None, 0, 5, 0, None, 0, 0, 0, one, None, 99, 99) == OK
        assert fn(None, None, 2, 0, 0, None, 0, 0, 0, one, None, 99, 99) == OK
        assert fn(None, None, 2, 5, 0, None, 7, 0, 0, one, None, 99, 99) == EMPTY
        assert fn(None, None, 2, 5, 0, None, 0, 4, 0, one, None, 99, 99) == EMPTY
        assert fn(None, None, 2, 5, 0, None, 7, 4, 0, one, None, 99, 99) == INVALID
        assert fn(None, None, 2, 5, 2, None, 8, 4, 0, one, None, 99, 99) == INVALID   # bins neither M nor M/2 + 1
        assert fn(None, None, 2, 5, 2, None, 6, 3, 0, one, None, 99, 99) == INVALID   # the one-sided form needs an even M
        assert fn(None, None, 2, 5, big, None, 2 * big, big, 0, one, None, 1 << 62, 99) == UNSUPPORTED
        assert fn(None, None, 2, 5, 3, None, 8, 4, 0, one, None, 99, 99) == HOP
        assert fn(None, None, 2, 1 << 61, 3, None, 8, 4, 2, one, None, 99, 99) == UNSUPPORTED
        assert fn(None, None, 2, 5, 3, None, 8, 4, 2, one, None, 12, 5) == MISMATCH   # full = 16
        assert fn(None, None, 2, 5, 4, None, 8, 4, 2, one, None, 17, 0) == MISMATCH
        assert fn(None, None, 2, 5, 3, None, 8, 4, 2, one, None, 12, 4) == NULL
        assert fn(None, p, 2, 5, 3, p, 8, 4, 2, one, p, 0, 16) == NULL
    assert lib.kofft_hip_set_pfb_fused(None, 1) == NULL


def test_python_errors_before_any_context():
    import kofft_amd
    from kofft_amd import pfb

    E = kofft_amd.FftError
    x = np.ones((2, 100), F)
    h = np.ones(16, F)
    S = np.ones((2, 3, 5), np.complex64)
    cases = [(lambda: pfb.analysis(x, h, 0), E.EmptyInput), (lambda: pfb.analysis(x, np.ones(0, F), 8), E.EmptyInput),
             (lambda: pfb.analysis(x, h, 7), E.InvalidValue), (lambda: pfb.analysis(x, h, 8, hop=0), E.InvalidHopSize),
             (lambda: pfb.analysis(np.ones((2, 0), F), h, 8), E.EmptyInput), (lambda: pfb.analysis(x, h, 8, lead=16), E.InvalidValue),
             (lambda: pfb.synthesis(S, h, 0, 4), E.EmptyInput), (lambda: pfb.synthesis(S, h, 7, 4), E.InvalidValue),
             (lambda: pfb.synthesis(S, h, 8, 0), E.InvalidHopSize), (lambda: pfb.synthesis(S, h, 16, 4), E.InvalidValue),
             (lambda: pfb.synthesis(S, h, 8, 4, out_first=20, out_len=5), E.MismatchedLengths),
             (lambda: pfb.reconstruction(h, np.ones(8, F), 8, 4), E.MismatchedLengths), (lambda: pfb.reconstruction(h, h, 8, 0), E.InvalidHopSize),
             (lambda: pfb.prototype(0, 4), E.EmptyInput), (lambda: pfb.prototype(8, 4, beta=-1.0), E.InvalidValue)]
    for call, code in cases:
        with pytest.raises(E) as e:
            call()
        assert e.value == E(code)
    for call in (lambda: pfb.analysis(np.ones((2, 2, 2), F), h, 8), lambda: pfb.synthesis(np.ones(8, np.complex64), h, 8, 4),
                 lambda: pfb.analysis(x, np.ones((2, 8), F), 8)):
        with pytest.raises(TypeError):
            call()
