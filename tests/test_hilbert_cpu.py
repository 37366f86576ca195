"""hilbert::hilbert_analytic (hilbert.rs:13-47) without a GPU: the test oracle against scipy's float64 analytic signal, an analytic
pin, and the argument checks of the C ABI and of the Python entry point, which come before any device is touched."""
import ctypes as C

import numpy as np
import pytest

from conftest import seeded
from hilbert_oracle import hilbert_ref


def _rel_l2(got, want):
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


@pytest.mark.parametrize("log2n", range(0, 17))
def test_oracle_matches_scipy(oracle, log2n):
    """The oracle's f32 result against scipy.signal.hilbert in float64.  The error grows with n through the reference's twiddle
    recurrence: about 2.6e-5 at n = 1024, 1.7e-4 at 4096, 1.1e-3 at 65536; the bound leaves a margin of 2x or more."""
    from scipy.signal import hilbert

    n = 1 << log2n
    x = seeded(7000 + log2n).uniform(-1, 1, (4, n)).astype(np.float32)
    got = hilbert_ref(x)
    assert got.dtype == np.complex64 and got.shape == x.shape
    want = hilbert(x.astype(np.float64), axis=-1)
    assert _rel_l2(got.astype(np.complex128), want) <= 1e-7 + 1e-7 * n, f"n={n}"


def test_oracle_analytic_pin(oracle):
    """cos(2 pi k t / n) has the analytic signal exp(i 2 pi k t / n)."""
    for n, k in [(8, 1), (64, 5), (1024, 100)]:
        t = np.arange(n)
        x = np.cos(2 * np.pi * k * t / n).astype(np.float32)[None, :]
        got = hilbert_ref(x)[0]
        assert np.max(np.abs(got - np.exp(2j * np.pi * k * t / n))) <= 1e-5 * max(1, np.log2(n)), f"n={n} k={k}"


def test_oracle_small_rows(oracle):
    """n = 1: (x, +0) (ifft returns early); n = 2: nothing doubled, nothing zeroed -- the input itself."""
    x = np.array([[3.5], [-0.0]], np.float32)
    got = hilbert_ref(x)
    assert got.real.tobytes() == x.tobytes() and got.imag.tobytes() == np.zeros_like(x).tobytes()
    x2 = np.array([[1.0, -2.0], [0.25, 4.0]], np.float32)
    assert np.array_equal(hilbert_ref(x2), x2.astype(np.complex64))


@pytest.mark.parametrize("entry", ["kofft_hip_hilbert_f32", "kofft_hip_hilbert_f32_dev"])
def test_abi_argument_order_null_context(hiplib, entry):
    """batch == 0 -> Ok, n == 0 -> EmptyInput, n not a power of two -> NonPowerOfTwoNoStd, n > 2^26 -> UNSUPPORTED, then the null
    context: each check before the next, none of them touching a device."""
    fn = getattr(hiplib, entry)
    null = C.c_void_p(None)
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    sz = C.c_size_t
    assert fn(null, p, p, sz(0), sz(1)) == 1
    assert fn(null, p, p, sz(12), sz(1)) == 2
    assert fn(null, p, p, sz(1 << 27), sz(1)) == -2
    assert fn(null, p, p, sz(8), sz(1)) == -3
    assert fn(null, p, p, sz(8), sz(0)) == 0
    assert fn(null, p, p, sz(0), sz(0)) == 0  # batch first
    assert fn(null, p, p, sz(3), sz(1)) == 2
    assert fn(null, p, p, sz(1 << 26), sz(1)) == -3  # the largest length is a valid request
    assert hiplib.kofft_hip_set_hilbert_fused(null, 0) == -3


def test_python_errors_need_no_device(monkeypatch):
    """hilbert_analytic raises EmptyInput / NonPowerOfTwoNoStd (hilbert.rs:14-19) before any context is created."""
    import kofft_amd
    from kofft_amd import api

    def no_device(*a, **k):
        raise AssertionError("a context was created")

    monkeypatch.setattr(api, "HipFftImpl", no_device)
    monkeypatch.setattr(api, "_hilbert_default", None)
    with pytest.raises(kofft_amd.FftError) as e:
        kofft_amd.hilbert_analytic([])
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.EmptyInput)
    with pytest.raises(kofft_amd.FftError) as e:
        kofft_amd.hilbert_analytic(np.ones(3, np.float32))
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.NonPowerOfTwoNoStd)
    with pytest.raises(kofft_amd.FftError) as e:
        kofft_amd.hilbert_analytic(np.ones((2, 0), np.float32))
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.EmptyInput)
    with pytest.raises(kofft_amd.FftError) as e:
        kofft_amd.hilbert_analytic(np.ones((4, 6), np.float32))
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.NonPowerOfTwoNoStd)
