"""cepstrum::real_cepstrum (cepstrum.rs:12-33) without a GPU: the test oracle's restatement of the libm crate's logf (constants, special
values, accuracy against float64), the oracle against numpy's float64 real cepstrum, an analytic pin, and the argument checks of the
C ABI and of the Python entry point, which come before any device is touched."""
import ctypes as C

import numpy as np
import pytest

from cepstrum_oracle import EPS, LG1, LG2, LG3, LG4, LN2_HI, LN2_LO, cepstrum_ref, libm_logf
from conftest import seeded


def _bits(v):
    return int(np.float32(v).view(np.uint32))


def test_libm_logf_constants():
    """The constants of libm 0.2 logf.rs by their hex comments, and cepstrum.rs:28's 1e-12 as an f32."""
    assert [_bits(c) for c in (LN2_HI, LN2_LO, LG1, LG2, LG3, LG4)] == [0x3F317180, 0x3717F7D1, 0x3F2AAAAA, 0x3ECCCE13, 0x3E91E9EE, 0x3E789E26]
    assert _bits(EPS) == 0x2B8CBCCC
    # the decimal spellings of the source give the same f32s
    assert [_bits(np.float32(d)) for d in (6.9313812256e-01, 9.0580006145e-06, 0.66666662693, 0.40000972152, 0.28498786688, 0.24279078841)] == \
        [_bits(c) for c in (LN2_HI, LN2_LO, LG1, LG2, LG3, LG4)]


def test_libm_logf_special_values():
    """1 -> +0; +inf -> +inf; NaN -> NaN; +-0 -> -inf; negatives (and -inf) -> NaN; subnormals through the 2^25 scaling."""
    x = np.array([1.0, np.inf, np.nan, 0.0, -0.0, -1.0, -np.inf, -1e-45], np.float32)
    got = libm_logf(x)
    assert _bits(got[0]) == 0  # +0, not -0
    assert got[1] == np.inf
    assert np.isnan(got[2])
    assert got[3] == -np.inf and got[4] == -np.inf
    assert np.isnan(got[5:]).all()
    sub = np.array([1e-45, 1e-40, 5.877472e-39, 1.1754942e-38], np.float32)  # the smallest subnormal .. the largest one
    assert (sub < np.float32(1.1754944e-38)).all()
    want = np.log(sub.astype(np.float64))
    assert np.all(np.abs(libm_logf(sub) - want) <= np.spacing(np.abs(want.astype(np.float32))))
    assert _bits(libm_logf(np.float32(2.0))[0]) == _bits(np.float32(np.log(2.0)))  # dk * LN2_HI + dk * LN2_LO at k = 1


def test_libm_logf_within_one_ulp_dense_stride():
    """Every 64th f32 in [1e-12f, FLT_MAX] (22 M values): within 1 ulp of float64 log (0.79 ulp at most on this stride)."""
    x = np.arange(_bits(EPS), 0x7F7FFFFF, 64, dtype=np.uint32).view(np.float32)
    got = libm_logf(x).astype(np.float64)
    want = np.log(x.astype(np.float64))
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    ulp[want == 0] = np.spacing(np.float32(0))
    err = np.abs(got - want) / ulp
    assert err.max() <= 1.0, f"worst {err.max():.3f} ulp at x = {x[np.argmax(err)]!r}"


@pytest.mark.parametrize("log2n", range(0, 17))
def test_oracle_matches_float64_cepstrum(oracle, log2n):
    """The oracle's f32 result against ifft(log(|fft(x)| + 1e-12)).real in float64.  The error grows with n through the reference's
    twiddle recurrence, as in test_hilbert_cpu.py: 1.1e-5 at n = 128, 3.4e-5 at 4096, 3.0e-4 at 32768 on these rows; the bound leaves a
    margin of 2.5x or more."""
    n = 1 << log2n
    x = seeded(8000 + log2n).uniform(-1, 1, (4, n)).astype(np.float32)
    got = cepstrum_ref(x)
    assert got.dtype == np.float32 and got.shape == x.shape
    want = np.fft.ifft(np.log(np.abs(np.fft.fft(x.astype(np.float64), axis=-1)) + 1e-12), axis=-1).real
    err = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    assert err <= 1e-6 + 2e-7 * n, f"n={n}: {err:.3e}"


def test_oracle_scaled_impulse(oracle):
    """a * delta has |X[k]| = |a| in every bin, so its real cepstrum is log|a| at index 0 and 0 elsewhere (1e-12 is below half an ulp
    of these magnitudes)."""
    for n in (1, 2, 8, 64, 1024, 4096):
        for a in (3.0, -0.5, 1e-3, 1.0):
            x = np.zeros((1, n), np.float32)
            x[0, 0] = a
            got = cepstrum_ref(x)[0]
            assert abs(float(got[0]) - np.log(abs(a))) <= 2 * abs(float(np.spacing(np.float32(np.log(abs(a)))))) + 1e-30, f"n={n} a={a}"
            assert np.all(np.abs(got[1:]) <= 1e-6), f"n={n} a={a}"


def test_oracle_n1_is_log_of_magnitude(oracle):
    """n = 1: the transform is nothing and ifft returns early: logf(sqrtf(x * x) + 1e-12f), with x * x overflowing to inf for
    |x| > 1.8e19 and underflowing to 0 (log(1e-12)) for tiny x."""
    x = np.array([[3.5], [-0.0], [-2.0], [3e19], [1e-30]], np.float32)
    got = cepstrum_ref(x)[:, 0]
    with np.errstate(over="ignore", under="ignore"):
        want = libm_logf(np.sqrt(x[:, 0] * x[:, 0]) + EPS)
    assert got.tobytes() == want.tobytes()
    assert got[3] == np.inf and got[4] == libm_logf(EPS)[0] and got[1] == libm_logf(EPS)[0]


@pytest.mark.parametrize("entry", ["kofft_hip_cepstrum_f32", "kofft_hip_cepstrum_f32_dev"])
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
    assert fn(null, C.c_void_p(None), p, sz(8), sz(1)) == -3
    assert hiplib.kofft_hip_set_cepstrum_fused(null, 0) == -3


def test_python_errors_need_no_device(monkeypatch):
    """real_cepstrum raises EmptyInput / NonPowerOfTwoNoStd (cepstrum.rs:13-18) before any context is created."""
    import kofft_amd
    from kofft_amd import api

    def no_device(*a, **k):
        raise AssertionError("a context was created")

    monkeypatch.setattr(api, "HipFftImpl", no_device)
    monkeypatch.setattr(api, "_cepstrum_default", None)
    with pytest.raises(kofft_amd.FftError) as e:
        kofft_amd.real_cepstrum([])
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.EmptyInput)
    with pytest.raises(kofft_amd.FftError) as e:
        kofft_amd.real_cepstrum(np.ones(3, np.float32))
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.NonPowerOfTwoNoStd)
    with pytest.raises(kofft_amd.FftError) as e:
        kofft_amd.real_cepstrum(np.ones((2, 0), np.float32))
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.EmptyInput)
    with pytest.raises(kofft_amd.FftError) as e:
        kofft_amd.real_cepstrum(np.ones((4, 6), np.float32))
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.NonPowerOfTwoNoStd)
    with pytest.raises(TypeError):
        kofft_amd.real_cepstrum(np.ones((2, 2, 4), np.float32))
