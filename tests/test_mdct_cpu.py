"""The fast DCT-IV, MDCT and IMDCT of DESIGN.md 5.32 without a GPU: the host table function, the oracle of tests/mdct_oracle.py against
float64 direct sums, the fold and unfold on small integers, perfect reconstruction with the three window helpers, the C entries'
argument checks in the header's order (a null context comes last, so none of them needs a device) and the Python module's errors, which
are raised before any context is created.

Accuracy bounds, relative L2 against float64 on uniform(-1, 1), 3 rows.  M = N / 2 a power of two: the project's bound for one
transform of M points, 1e-6 + 2e-7 M (tests/test_convolve_cpu.py); measured 3.6e-7 at N = 64, 9.4e-6 at 1024, 8.6e-5 at 8192.  M not a
power of two (the oracle's Bluestein arm): twice the worst of eight seeds -- N = 6: 1.48e-7, N = 240: 1.33e-5, N = 960: 6.25e-5.  Round
trip imdct(mdct(x)) against x, twice the worst of five seeds and three windows (the windows agree to 1 %): see ROUND_TRIP."""
import ctypes as C

import numpy as np
import pytest

from conftest import seeded
import mdct_oracle as mo

F = np.float32
# N -> bound of one dct4_fast against float64 where N / 2 is not a power of two: 2 x the worst of seeds 0 .. 7
BLUESTEIN = {6: 2 * 1.48e-7, 240: 2 * 1.33e-5, 960: 2 * 6.25e-5}
# N -> bound of the round trip: 2 x the worst of seeds 100 .. 104 and the three windows on the CPU oracle
ROUND_TRIP = {2: 2 * 1.6e-7, 4: 2 * 1.5e-7, 64: 2 * 7.11e-7, 240: 2 * 5.47e-6, 960: 2 * 7.49e-5, 1024: 2 * 1.84e-5, 8192: 2 * 1.7e-4}


def bound(n: int) -> float:
    m = n // 2
    return 1e-6 + 2e-7 * m if m & (m - 1) == 0 else BLUESTEIN[n]


def rel(a, b) -> float:
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def dct4_f64(u):
    n = u.shape[-1]
    i = np.arange(n) + 0.5
    return u.astype(np.float64) @ np.cos(np.pi / n * np.outer(i, i))


def mdct_f64(g):
    """[..., 2N] windowed frames -> [..., N]: sum_i g[i] cos(pi / N (i + 1/2 + N/2)(k + 1/2))"""
    n = g.shape[-1] // 2
    return g.astype(np.float64) @ np.cos(np.pi / n * np.outer(np.arange(2 * n) + 0.5 + n / 2, np.arange(n) + 0.5))


def windows(n):
    from kofft_amd import mdct as km

    return [("sine", km.sine_window(n)), ("vorbis", km.vorbis_window(n)), ("kbd", km.kbd_window(n, 4.0))]


@pytest.mark.parametrize("n", [2, 6, 64, 240, 8192])
def test_tables(n):
    c, d = mo.tables(n)
    m = n // 2
    a = -np.pi * (4 * np.arange(m, dtype=np.float64) + 1) / (4 * n)
    b = -np.pi * np.arange(m, dtype=np.float64) / n
    for got, ang, fn in ((c.real, a, np.cos), (c.imag, a, np.sin), (d.real, b, np.cos), (d.imag, b, np.sin)):
        want = fn(ang).astype(F)
        assert got.dtype == F and np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want)).astype(np.float64))
    assert d[0] == 1.0 + 0.0j


def test_table_checks():
    from kofft_amd import _lib

    lib = _lib.load()
    buf = np.zeros(8, F)
    assert lib.kofft_hip_dct4_table_f32(0, C.c_void_p(buf.ctypes.data)) == 1  # EMPTY_INPUT
    assert lib.kofft_hip_dct4_table_f32(3, C.c_void_p(buf.ctypes.data)) == 6  # INVALID_VALUE
    assert lib.kofft_hip_dct4_table_f32(4, None) == -3


@pytest.mark.parametrize("n", [2, 4, 6, 64, 128, 240, 960, 1024, 8192])
def test_dct4_ref_against_float64(oracle, n):
    u = seeded(11000 + n).uniform(-1, 1, (3, n)).astype(F)
    err = rel(mo.dct4_ref(u), dct4_f64(u))
    print(f"N={n}: relative L2 error {err:.3g}, bound {bound(n):.3g}")
    assert err <= bound(n)


@pytest.mark.parametrize("n", [2, 4, 64, 240, 1024])
def test_mdct_and_imdct_ref_against_float64(oracle, n):
    rows, nx = 3, 5 * n + 3
    x = seeded(11100 + n).uniform(-1, 1, (rows, nx)).astype(F)
    w = windows(n)[0][1]
    for lead in sorted({0, 1, n, 2 * n - 1}):
        frames = -(-(nx + lead) // n)
        X = mo.mdct_ref(x, w, lead, frames)
        err = rel(X, mdct_f64(mo.windowed_frames(x, w, lead, frames)))
        print(f"N={n} lead={lead}: mdct relative L2 error {err:.3g}, bound {bound(n):.3g}")
        assert err <= bound(n)
    # the IMDCT: y_f[i] = sum_k X[k] cos(pi / N (i + 1/2 + N/2)(k + 1/2)), windowed, overlap-added, scaled
    y = X.astype(np.float64) @ np.cos(np.pi / n * np.outer(np.arange(n) + 0.5, np.arange(2 * n) + 0.5 + n / 2)) * w.astype(np.float64)
    full = np.zeros((rows, (frames + 1) * n))
    for f in range(frames):
        full[:, f * n:(f + 2) * n] += y[:, f]
    full *= float(F(2.0 / n))
    err = rel(mo.imdct_ref(X, w, 2.0 / n), full)
    print(f"N={n}: imdct relative L2 error {err:.3g}, bound {bound(n):.3g}")
    assert err <= bound(n)


@pytest.mark.parametrize("n", [2, 4])
def test_fold_and_unfold_on_integers(n):
    g = np.arange(1, 2 * n + 1, dtype=F)
    want_u = {2: [-3 - 4, 1 - 2], 4: [-6 - 7, -5 - 8, 1 - 4, 2 - 3]}[n]
    assert mo.fold(g[None])[0].tolist() == want_u
    v = np.arange(1, n + 1, dtype=F)
    want_y = {2: [2, -2, -1, -1], 4: [3, 4, -4, -3, -2, -1, -1, -2]}[n]
    assert mo.unfold(v[None])[0].tolist() == want_y
    # the fold is the MDCT's aliasing: mdct(g) == dct4(fold(g)) in float64 too
    assert np.allclose(mdct_f64(g[None]), dct4_f64(mo.fold(g[None])), atol=1e-12)


@pytest.mark.parametrize("n", [2, 4, 64, 240, 960, 1024, 8192])
def test_windows_and_round_trip(oracle, n):
    for name, w in windows(n):
        w64 = w.astype(np.float64)
        assert w.dtype == F and w.shape == (2 * n,)
        assert np.abs(w64[:n] ** 2 + w64[n:] ** 2 - 1.0).max() <= 1e-6, name
        worst = 0.0
        for seed in range(100, 105):
            x = np.random.default_rng(seed).uniform(-1, 1, (3, 5 * n + 3)).astype(F)
            frames = -(-x.shape[1] // n) + 1
            full = mo.imdct_ref(mo.mdct_ref(x, w, n, frames), w, 2.0 / n)
            worst = max(worst, rel(full[:, n:n + x.shape[1]], x))
        print(f"N={n} {name}: round trip relative L2 error {worst:.3g}, bound {ROUND_TRIP[n]:.3g}")
        assert worst <= ROUND_TRIP[n]


def test_c_checks_in_header_order():
    """Each call trips one check and would trip every later one as well; the null context is the last."""
    from kofft_amd import _lib

    lib = _lib.load()
    OK, EMPTY, MISMATCH, INVALID, UNSUPPORTED, NULL = 0, 1, 3, 6, -2, -3
    buf = np.zeros(64, F)
    p = C.c_void_p(buf.ctypes.data)
    big = (1 << 26) + 2  # N / 2 = 2^25 + 1: not a power of two and above 2^25
    for fn in (lib.kofft_hip_dct4_fast_f32, lib.kofft_hip_dev_dct4_fast_f32):
        assert fn(None, None, None, 0, 0) == OK
        assert fn(None, None, None, 0, 1) == EMPTY
        assert fn(None, None, None, 3, 1) == INVALID
        assert fn(None, None, None, big, 1) == UNSUPPORTED
        assert fn(None, None, None, 4, 1 << 62) == UNSUPPORTED
        assert fn(None, p, p, 4, 1) == NULL
    for fn in (lib.kofft_hip_mdct_f32, lib.kofft_hip_dev_mdct_f32):
        # (ctx, x, rows, nx, row_stride, window, N, lead, out, frames)
        assert fn(None, None, 0, 0, 0, None, 0, 99, None, 5) == OK
        assert fn(None, None, 2, 0, 0, None, 0, 99, None, 0) == OK
        assert fn(None, None, 2, 0, 0, None, 0, 99, None, 5) == EMPTY
        assert fn(None, None, 2, 0, 0, None, 3, 99, None, 5) == INVALID
        assert fn(None, None, 2, 0, 0, None, big, 1 << 40, None, 5) == UNSUPPORTED
        assert fn(None, None, 2, 0, 0, None, 4, 99, None, 5) == EMPTY      # nx == 0
        assert fn(None, None, 2, 10, 5, None, 4, 8, None, 5) == INVALID     # lead >= 2N
        assert fn(None, None, 2, 10, 5, None, 4, 7, None, 5) == INVALID     # row_stride < nx
        assert fn(None, None, 1, 10, 5, None, 4, 7, None, 1 << 61) == UNSUPPORTED
        assert fn(None, None, 1, 10, 5, None, 4, 7, None, 5) == NULL        # (rows == 1: the stride is ignored)
        assert fn(None, p, 2, 10, 10, p, 4, 7, p, 5) == NULL
    for fn in (lib.kofft_hip_imdct_f32, lib.kofft_hip_dev_imdct_f32):
        # (ctx, coef, rows, frames, window, N, scale, out, out_first, out_len)
        one = C.c_float(1.0)
        assert fn(None, None, 0, 5, None, 0, one, None, 99, 99) == OK
        assert fn(None, None, 2, 0, None, 0, one, None, 99, 99) == OK
        assert fn(None, None, 2, 5, None, 0, one, None, 99, 0) == OK
        assert fn(None, None, 2, 5, None, 0, one, None, 99, 99) == EMPTY
        assert fn(None, None, 2, 5, None, 3, one, None, 99, 99) == INVALID
        assert fn(None, None, 2, 5, None, big, one, None, 1 << 62, 99) == UNSUPPORTED
        assert fn(None, None, 2, 1 << 61, None, 4, one, None, 99, 99) == UNSUPPORTED
        assert fn(None, None, 2, 5, None, 4, one, None, 20, 5) == MISMATCH   # full = 24
        assert fn(None, None, 2, 5, None, 4, one, None, 25, 1) == MISMATCH
        assert fn(None, None, 2, 5, None, 4, one, None, 20, 4) == NULL
        assert fn(None, p, 2, 5, p, 4, one, p, 0, 24) == NULL
    assert lib.kofft_hip_set_mdct_fused(None, 1) == NULL


def test_python_errors_before_any_context():
    import kofft_amd
    from kofft_amd import mdct as km

    E = kofft_amd.FftError
    x = np.ones((2, 100), F)
    cases = [(lambda: km.mdct(x, 0), E.EmptyInput), (lambda: km.mdct(x, 7), E.InvalidValue),
             (lambda: km.mdct(x, 8, window=np.ones(15, F)), E.MismatchedLengths), (lambda: km.mdct(x, 8, lead=16), E.InvalidValue),
             (lambda: km.mdct(np.ones((2, 0), F), 8), E.EmptyInput), (lambda: km.imdct(np.ones((2, 3, 7), F)), E.InvalidValue),
             (lambda: km.imdct(np.ones((2, 3, 8), F), window=np.ones(8, F)), E.MismatchedLengths),
             (lambda: km.imdct(np.ones((2, 3, 8), F), length=25), E.MismatchedLengths), (lambda: km.dct4(np.ones((2, 5), F)), E.InvalidValue),
             (lambda: km.dct4(np.ones((2, 0), F)), E.EmptyInput), (lambda: km.sine_window(3), E.InvalidValue),
             (lambda: km.kbd_window(0), E.EmptyInput)]
    for call, code in cases:
        with pytest.raises(E) as e:
            call()
        assert e.value == E(code)
    for call in (lambda: km.mdct(np.ones((2, 2, 2), F), 8), lambda: km.imdct(np.ones(8, F)), lambda: km.dct4(F(1.0))):
        with pytest.raises(TypeError):
            call()
