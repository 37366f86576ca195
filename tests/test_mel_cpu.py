"""The mel filterbank and MFCC on the host side (no GPU): the argument checks of the C ABI in their order through a null context, the
reference's own three tests restated on the oracle (tests/mel_oracle.py), kofft_hip_mel_bins_f32 against the f32 formula and against
the float64 floors at the seven settings whose edges keep clear of the integers, the Python module's errors before any device, and the
edge helper and the plan builder in a stand-alone program under sanitizers."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mel_oracle as mo

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
# smallest distance of an exact edge 1 .. M + 1 to an integer at each setting (mel_oracle.SETTINGS, same order)
CLEARANCE = [1.9e-2, 1.3e-2, 9.2e-3, 5.2e-3, 3.7e-3, 2.8e-2, 1.5e-3]


def _u64(v):
    return np.ascontiguousarray(v, np.uint64)


def _lib_bins(hiplib, rate, n_fft, filters):
    out = np.full(filters + 2, 7, np.uint64)
    assert hiplib.kofft_hip_mel_bins_f32(rate, n_fft, filters, C.c_void_p(out.ctypes.data)) == 0
    return [int(v) for v in out]


def test_argument_checks_in_order_with_a_null_context(hiplib):
    """include/kofft_hip.h: rows == 0, num_coeffs > num_mel, null bins, bins out of order, the bounds, null data or context -- no
    context needed; the overlap check (device forms) comes after the null context and is tested on the GPU."""
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    good = _u64([0, 2, 4, 6])
    bad = _u64([0, 4, 2, 6])
    long_bins = _u64(np.arange(4099))
    g, b, lb = (C.c_void_p(a.ctypes.data) for a in (good, bad, long_bins))
    big = (1 << 24) + 1
    for fb in (hiplib.kofft_hip_mel_filterbank_f32, hiplib.kofft_hip_dev_mel_filterbank_f32):
        assert fb(None, None, None, big, 0, None, 5000) == 0  # rows == 0 before everything
        assert fb(None, p, p, 8, 1, None, 2) == -3            # null bins
        assert fb(None, None, None, big, 1, b, 2) == 6        # order before the bounds
        assert fb(None, None, None, big, 1, g, 2) == -2       # n_fft > 2^24 before the pointers
        assert fb(None, None, None, 8, 1, lb, 4097) == -2     # num_mel > 4096
        assert fb(None, None, None, 8, 1, g, 2) == -3         # then null data and context
        assert fb(None, p, p, 8, 1, g, 2) == -3
        assert fb(None, p, p, 8, 1, g, 0) == -3               # num_mel == 0 is a valid call: the null context is reported
    for mf in (hiplib.kofft_hip_mfcc_f32, hiplib.kofft_hip_dev_mfcc_f32):
        assert mf(None, None, None, big, 0, None, 2, 9) == 0  # rows == 0 before num_coeffs > num_mel
        assert mf(None, None, None, big, 1, None, 2, 3) == 6  # num_coeffs > num_mel before null bins
        assert mf(None, p, p, 8, 1, None, 2, 2) == -3         # null bins
        assert mf(None, None, None, big, 1, b, 2, 2) == 6     # order before the bounds
        assert mf(None, None, None, big, 1, g, 2, 2) == -2
        assert mf(None, None, None, 8, 1, lb, 4097, 13) == -2
        assert mf(None, None, None, 8, 1, g, 2, 2) == -3
        assert mf(None, p, p, 8, 1, g, 2, 0) == -3
    assert hiplib.kofft_hip_set_mfcc_fused(None, 0) == -3
    mb = hiplib.kofft_hip_mel_bins_f32
    assert mb(16000.0, 32, 4097, g) == -2 and mb(16000.0, 32, 8, None) == -3


@pytest.mark.parametrize("setting,clear", list(zip(mo.SETTINGS, CLEARANCE)))
def test_mel_bins_are_the_f32_formula_and_the_float64_floors(hiplib, setting, clear):
    rate, n_fft, filters = setting
    got = _lib_bins(hiplib, float(rate), n_fft, filters)
    assert got == mo.ref_bins(rate, n_fft, filters)
    exact = mo.edges_f64(rate, n_fft, filters)
    dist = min(abs(e - round(e)) for e in exact[1:])
    print(f"{setting}: smallest distance of an edge to an integer {dist:.2e}")
    assert dist >= 0.9 * clear, "the setting is not the one the issue measured"
    assert got == [int(np.floor(e)) for e in exact]
    assert got[0] == 0 and all(b >= a for a, b in zip(got, got[1:]))


def test_mel_bins_saturate(hiplib):
    """`floorf(..) as usize`: NaN and negatives give 0, infinity the largest value."""
    assert _lib_bins(hiplib, float("nan"), 32, 3) == [0] * 5
    assert _lib_bins(hiplib, -16000.0, 32, 3) == mo.ref_bins(-16000.0, 32, 3)
    got = _lib_bins(hiplib, 3e38, 1 << 24, 2)
    assert got == mo.ref_bins(3e38, 1 << 24, 2) and got[-1] == mo.U64_MAX
    assert _lib_bins(hiplib, 16000.0, 0, 0) == [0, 0]


def test_the_references_own_tests_on_the_oracle(hiplib):
    """cepstrum.rs:121-148 restated: the batch of two frames gives 2 x 4 finite coefficients (the device repeats it in
    tests/test_gpu_mfcc.py); num_coeffs = 20 > 8 is InvalidValue; 8 magnitudes at (8000, 40) have no live filter: 40 energies of +0."""
    frames = np.stack([np.full(32, 1.0, F), np.full(32, 0.5, F)])
    bins = _lib_bins(hiplib, 16000.0, 32, 8)
    got = mo.mfcc(frames, bins, 4)
    assert got.shape == (2, 4) and got.dtype == F and np.isfinite(got).all()
    p = C.c_void_p(frames.ctypes.data)
    b = _u64(bins)
    assert hiplib.kofft_hip_mfcc_f32(None, p, p, 32, 1, C.c_void_p(b.ctypes.data), 8, 20) == 6
    bins = _lib_bins(hiplib, 8000.0, 8, 40)
    assert not any(mo.live(bins)), bins
    e = mo.energies(np.ones((1, 8), F), bins)
    assert e.shape == (1, 40) and e.tobytes() == np.zeros((1, 40), F).tobytes()


def test_oracle_on_hand_made_edges():
    """The oracle's own sanity on cases small enough to do by hand: one filter [0, 2, 4] on (1, 2, 3, 4) is 0/2*1 + 1/2*2 + 2/2*3 +
    1/2*4 = 6; terms past the row are skipped with the denominators kept; a dead filter stays +0."""
    x = np.array([[1.0, 2.0, 3.0, 4.0]], F)
    assert mo.energies(x, [0, 2, 4])[0, 0] == F(6.0)
    assert mo.energies(x, [0, 2, 8])[0, 0] == F(4.0) + (F(5.0) / F(6.0)) * F(4.0)  # 0 + 1 + (6/6) * 3, then (5/6) * 4
    assert mo.energies(x, [0, 0, 4, 4]).tobytes() == np.zeros((1, 2), F).tobytes()
    assert mo.energies(np.zeros((3, 0), F), [0, 2, 4]).tobytes() == np.zeros((3, 1), F).tobytes()
    lm = mo.mfcc(np.zeros((1, 0), F), [0, 2, 4, 6], 2)
    assert lm.shape == (1, 2) and np.isfinite(lm).all()


def test_python_errors_before_any_device():
    import kofft_amd
    from kofft_amd import api, mfcc

    before = api._direct_default
    row = np.ones(32, F)
    with pytest.raises(kofft_amd.FftError) as e:
        mfcc.mfcc(row, 16000.0, 8, 20)
    assert e.value.code == 6
    with pytest.raises(kofft_amd.FftError):
        mfcc.mfcc_batch([row, row[:8]], 16000.0, 8, 9)
    with pytest.raises(kofft_amd.DeviceError):
        mfcc.mel_filterbank(row, 16000.0, 4097)
    with pytest.raises(kofft_amd.FftError):
        mfcc.mel_filterbank(row, 16000.0, 2, bins=[0, 5, 3, 9])
    with pytest.raises(kofft_amd.FftError):
        mfcc.mel_filterbank(row, 16000.0, 2, bins=[0, 3, 9])  # not num_filters + 2 edges
    with pytest.raises(TypeError):
        mfcc.mel_filterbank(row, 16000.0, 2, bins=[0.0, 1.0, 2.0, 3.0])
    with pytest.raises(TypeError):
        mfcc.mfcc_batch([np.ones((2, 8), F)], 16000.0, 4, 2)
    assert mfcc.mfcc(row, 16000.0, 8, 0).shape == (0,)
    assert mfcc.mel_filterbank(row, 16000.0, 0).shape == (0,)
    assert mfcc.mfcc_batch([], 16000.0, 8, 4) == []
    assert [int(v) for v in mfcc.mel_bins(16000.0, 32, 8)] == mo.ref_bins(16000, 32, 8)
    assert api._direct_default is before, "a context was created before the errors"


def test_mel_plan_under_asan_ubsan(tmp_path):
    """The edge helper and the plan builder in a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer."""
    exe = tmp_path / "sanitize_mel_plan"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-ffp-contract=off"]
    subprocess.run(["g++", "-std=c++17", *flags, str(ROOT / "tests" / "cpp" / "sanitize_mel_plan.cpp"),
                    str(ROOT / "kofft_amd" / "csrc" / "tables.cpp"), "-lm", "-pthread", "-o", str(exe)], check=True, capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert res.returncode == 0, res.stdout + res.stderr
    assert "0 problems" in res.stdout
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
