"""The windows beyond Hann (no GPU: they are host code like kofft_hip_hann_f32): kofft_hip_window_f32 and kofft_amd.window against
tests/window_oracle.py bit for bit (NaN compared as NaN), the reference's clamp test, the pinned edge cases and the argument checks."""
import ctypes as C

import numpy as np
import pytest

import window_oracle as wo

F = np.float32
LENS = [0, 1, 2, 3, 8, 255, 256, 1000, 4096]
BETAS = [0.0, 5.0, 8.6]
ALPHAS = [-0.5, 0.0, 0.5, 1.0, 1.5, float("nan")]


def _lib_window(hiplib, kind, length, param=0.0):
    out = np.full(length, 7.0, F)
    rc = hiplib.kofft_hip_window_f32(wo.KINDS.index(kind), length, param, C.c_void_p(out.ctypes.data) if length else None)
    assert rc == 0, (kind, length, param, rc)
    return out


def _same(got, want):
    """Bit for bit, except that any NaN matches any NaN."""
    ng, nw = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(ng, nw) and got[~ng].tobytes() == want[~nw].tobytes()


@pytest.mark.parametrize("length", LENS)
@pytest.mark.parametrize("kind", ["hamming", "blackman", "bartlett", "bohman", "nuttall"])
def test_parameterless_windows_bit_for_bit(hiplib, kind, length):
    from kofft_amd import window

    want = wo.window(kind, length)
    assert _same(_lib_window(hiplib, kind, length), want)
    assert _same(getattr(window, kind)(length), want)


@pytest.mark.parametrize("length", LENS)
@pytest.mark.parametrize("beta", BETAS)
def test_kaiser_bit_for_bit(hiplib, beta, length):
    from kofft_amd import window

    if length == 0:  # the reference underflows len - 1: EMPTY_INPUT here, a refusal in the oracle
        assert hiplib.kofft_hip_window_f32(2, 0, beta, None) == 1
        with pytest.raises(ValueError):
            wo.window("kaiser", 0, beta)
        return
    want = wo.window("kaiser", length, beta)
    assert _same(_lib_window(hiplib, "kaiser", length, beta), want)
    assert _same(window.kaiser(length, beta), want)


@pytest.mark.parametrize("length", LENS)
@pytest.mark.parametrize("alpha", ALPHAS)
def test_tukey_bit_for_bit(hiplib, alpha, length):
    from kofft_amd import window

    want = wo.window("tukey", length, alpha)
    assert _same(_lib_window(hiplib, "tukey", length, alpha), want)
    assert _same(window.tukey(length, alpha), want)


def test_tukey_alpha_clamp(hiplib):
    """window_more.rs:82-89."""
    from kofft_amd import window

    assert window.tukey(8, -0.5).tobytes() == window.tukey(8, 0.0).tobytes()
    assert window.tukey(8, 1.5).tobytes() == window.tukey(8, 1.0).tobytes()
    assert window.tukey(8, 1.0).tobytes() != window.tukey(8, 0.0).tobytes()


def test_edge_cases_pinned_in_the_header(hiplib):
    import kofft_amd
    from kofft_amd import window

    # len == 1: the reference divides zero by zero in these four
    for kind in ("bartlett", "bohman", "nuttall"):
        assert np.isnan(_lib_window(hiplib, kind, 1)).all(), kind
    assert np.isnan(_lib_window(hiplib, "kaiser", 1, 5.0)).all()
    assert _lib_window(hiplib, "tukey", 1, 0.5).tolist() == [1.0]
    assert _lib_window(hiplib, "hamming", 1)[0] == F(0.54) - F(0.46)
    # kaiser(0, .) underflows len - 1 in the reference
    assert hiplib.kofft_hip_window_f32(2, 0, 5.0, None) == 1
    with pytest.raises(kofft_amd.FftError) as e:
        window.kaiser(0, 5.0)
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.EmptyInput)
    # tukey: a NaN alpha survives the clamp, its edge saturates to 0 -> all ones, like alpha <= 0
    for alpha in (float("nan"), 0.0, -0.0, -3.0, float("-inf")):
        assert _lib_window(hiplib, "tukey", 9, alpha).tolist() == [1.0] * 9, alpha
    assert window.tukey(9, float("inf")).tobytes() == window.tukey(9, 1.0).tobytes()
    # the reference's own pins (window.rs:110-133, window_more.rs:70-79)
    w = window.kaiser(9, 5.0)
    assert abs(w[4] - 1.0) < 1e-6 and np.all(np.abs(w - w[::-1]) < 1e-6) and np.isfinite(w).all()
    assert np.all((window.hamming(8) >= 0) & (window.hamming(8) <= 1))
    assert np.all((window.blackman(8) >= -1e-6) & (window.blackman(8) <= 1))
    assert all(getattr(window, k)(8).shape == (8,) for k in ("bartlett", "bohman", "nuttall"))
    assert window.hann(8).tobytes() == kofft_amd.hann(8).tobytes()


def test_argument_checks_in_order(hiplib):
    import kofft_amd
    from kofft_amd import window

    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)
    f = hiplib.kofft_hip_window_f32
    assert f(-1, 0, 0.0, None) == 6 and f(7, 4, 0.0, p) == 6  # the kind before everything
    for kind in range(7):
        assert f(kind, 0, 0.0, None) == (1 if kind == 2 else 0)  # len == 0 before the pointer
        assert f(kind, 4, 0.5, None) == -3
        assert f(kind, 4, 0.5, p) == 0
    with pytest.raises(kofft_amd.FftError):
        window.window("welch", 8)
    with pytest.raises(kofft_amd.FftError):
        window.window(9, 8)
    with pytest.raises(ValueError):
        window.hamming(-1)
    assert window.window(0, 8).tobytes() == window.hamming(8).tobytes()
