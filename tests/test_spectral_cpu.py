"""czt::czt_f32 and goertzel::goertzel_f32 on the host side (no GPU): the numpy oracle against a scalar transcription of the Rust
loops and against float64, the reference's own known answers, the library's host tables against the oracle bit for bit, the argument
checks of the C ABI and of the Python modules, the machine code of the new kernels (nothing fused) and the new host code under
AddressSanitizer + UBSan."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import spectral_oracle as so
from conftest import seeded

ROOT = Path(__file__).resolve().parent.parent
SETS = ("dft", "zoom", "spiral", "a_zero", "grow")
FINITE_SETS = ("dft", "zoom", "a_zero")  # spiral underflows and grow overflows: no float64 comparison means anything there


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("n,m", [(0, 3), (1, 1), (2, 5), (7, 4), (33, 9)])
def test_czt_oracle_is_the_scalar_transcription(name, n, m):
    w, a = so.param_sets(m)[name]
    x = seeded(11000 + 10 * n + m).uniform(-1, 1, (2, n)).astype(np.float32)
    got = so.czt(x, m, w, a)
    for r in range(2):
        assert got[r].tobytes() == so.czt_scalar(x[r], m, w, a).tobytes(), f"{name} n={n} m={m} row {r}"
    assert so.czt_table(n, m, w, a).shape == (n, 2 * m)


def test_czt_oracle_special_values_match_the_scalar_form():
    from rowcheck import assert_rows_equal

    x = np.array([1.0, np.inf, -0.0, np.nan, 1e-45, -3e38, 2.0], np.float32)
    for name in SETS:
        w, a = so.param_sets(6)[name]
        assert_rows_equal(so.czt(x, 6, w, a), so.czt_scalar(x, 6, w, a), name, nan_safe=True)  # (a NaN's sign is the platform's)


@pytest.mark.parametrize("n", [1, 2, 3, 31, 100])
def test_goertzel_oracle_is_the_scalar_transcription(n):
    x = seeded(11500 + n).uniform(-1, 1, (3, n)).astype(np.float32)
    x[1, 0] = np.inf
    freqs = [0.0, 1000.0, 4000.0, 9000.0, -500.0]
    got = so.goertzel(x, 8000.0, freqs)
    for r in range(3):
        for j, f in enumerate(freqs):
            want = so.goertzel_scalar(x[r], 8000.0, f)
            assert got[r, j].tobytes() == np.float32(want).tobytes() or (np.isnan(got[r, j]) and np.isnan(want)), (n, r, f)


def test_reference_known_answers():
    """czt.rs:60-81 and goertzel.rs:65-76 on the oracle."""
    w = (np.float32(np.cos(np.float32(-2.0 * np.float32(np.pi) / 4.0))), np.float32(np.sin(np.float32(-2.0 * np.float32(np.pi) / 4.0))))
    y = so.czt(np.array([1, 0, 0, 0], np.float32), 4, w, (1.0, 0.0))
    assert abs(y[0].real - 1.0) < 1e-5
    y = so.czt(np.array([0, 1], np.float32), 2, (0.0, 1.0), (0.5, 0.0))
    assert abs(y[0].real - 2.0) < 1e-5 and abs(y[0].imag) < 1e-5
    assert abs(y[1].real) < 1e-5 and abs(y[1].imag - 2.0) < 1e-5
    i = np.arange(100, dtype=np.float32)
    sig = np.sin(np.float32(2.0) * np.float32(np.pi) * np.float32(1000.0) * i / np.float32(8000.0)).astype(np.float32)
    assert so.goertzel(sig, 8000.0, [1000.0])[0] > 0.0


def test_python_errors_mirror_the_reference_before_any_device():
    """goertzel.rs:78-93 (EmptyInput, then InvalidValue) and the bounds, with no context created."""
    import kofft_amd
    from kofft_amd import api, czt, goertzel

    before = api._direct_default
    with pytest.raises(kofft_amd.FftError) as e:
        goertzel.goertzel_f32(np.zeros(0, np.float32), 1.0, 1.0)
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.EmptyInput)
    with pytest.raises(kofft_amd.FftError) as e:
        goertzel.goertzel_f32(np.zeros(0, np.float32), 0.0, 1.0)  # the empty input is reported first
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.EmptyInput)
    with pytest.raises(kofft_amd.FftError) as e:
        goertzel.goertzel_f32(np.array([1.0, 2.0], np.float32), 0.0, 1.0)
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.InvalidValue)
    with pytest.raises(kofft_amd.DeviceError):
        goertzel.goertzel_f32(np.zeros(4, np.float32), 1.0, np.zeros(1025, np.float32))
    with pytest.raises(kofft_amd.DeviceError):
        czt.czt_f32(np.zeros(4097, np.float32), 4, 1.0, 1.0)
    with pytest.raises(kofft_amd.DeviceError):
        czt.czt_f32(np.zeros(4, np.float32), 4097, 1.0, 1.0)
    with pytest.raises(TypeError):
        czt.czt_f32(np.zeros((1, 2, 3), np.float32), 4, 1.0, 1.0)
    assert czt.czt_f32(np.zeros(4, np.float32), 0, 1.0, 1.0).shape == (0,)
    assert czt.czt_f32(np.zeros((0, 4), np.float32), 3, 1.0, 1.0).shape == (0, 3)
    import torch

    class OnDevice:  # stands for a device tensor where there is no device: the empty results stay tensors
        shape, is_cuda, device = (0, 4), True, torch.device("cpu")

        def data_ptr(self):
            return 0

    e = czt.czt_f32(OnDevice(), 3, 1.0, 1.0)
    assert isinstance(e, torch.Tensor) and tuple(e.shape) == (0, 3) and e.dtype == torch.complex64
    e = goertzel.goertzel_f32(OnDevice(), 8000.0, [1.0, 2.0])
    assert isinstance(e, torch.Tensor) and tuple(e.shape) == (0, 2) and e.dtype == torch.float32
    assert api._direct_default is before, "a context was created before the errors"


# ---- the library's host tables ----------------------------------------------------------------------------------------------------
def _lib_table(hiplib, n, m, w, a):
    (wr, wi), (ar, ai) = so._pair(w), so._pair(a)
    c = np.full((n, 2 * m), 7.0, np.float32)
    assert hiplib.kofft_hip_czt_table_f32(n, m, wr, wi, ar, ai, C.c_void_p(c.ctypes.data)) == 0
    return c


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("n,m", [(1, 1), (4, 4), (17, 5), (5, 17), (64, 63), (100, 300)])
def test_host_czt_table_is_the_oracle_bit_for_bit(hiplib, name, n, m):
    from rowcheck import assert_rows_equal

    w, a = so.param_sets(m)[name]
    assert_rows_equal(_lib_table(hiplib, n, m, w, a), so.czt_table(n, m, w, a), f"{name} n={n} m={m}", nan_safe=True)


def _lib_coeff(hiplib, n, rate, freqs):
    f = np.ascontiguousarray(freqs, np.float32)
    out = np.empty(f.size, np.float32)
    rc = hiplib.kofft_hip_goertzel_coeff_f32(n, C.c_float(rate), C.c_void_p(f.ctypes.data), f.size, C.c_void_p(out.ctypes.data))
    return rc, out


@pytest.mark.parametrize("n", [1, 2, 100, 4099, 1 << 20])
def test_host_goertzel_coefficients_are_the_oracle_bit_for_bit(hiplib, n):
    freqs = np.array([0.0, 1000.0, 4000.0, 7999.0, -250.0, -8000.0, 8000.0, 20000.0, 1e9, 0.3, np.inf], np.float32)  # k < 0, k > n too
    rc, got = _lib_coeff(hiplib, n, 8000.0, freqs)
    want = so.goertzel_coeff(n, 8000.0, freqs)
    assert rc == 0 and np.array_equal(np.isnan(got), np.isnan(want))
    assert got[~np.isnan(got)].tobytes() == want[~np.isnan(want)].tobytes()
    rc, got = _lib_coeff(hiplib, n, float("nan"), freqs)  # a NaN rate passes `<= 0.0` (goertzel.rs:20)
    assert rc == 0 and np.all(np.isnan(got)) and np.all(np.isnan(so.goertzel_coeff(n, np.nan, freqs)))


# ---- float64 sanity of the oracle -----------------------------------------------------------------------------------------------------
def _f64_czt(x, m, w, a):
    """sum_i x[i] * a^-i * w^(i k) in float64 from the f32 w and a, and sum_i |term|."""
    (wr, wi), (ar, ai) = so._pair(w), so._pair(a)
    w64, a64 = complex(float(wr), float(wi)), complex(float(ar), float(ai))
    n = x.shape[1]
    i = np.arange(n)[:, None]
    k = np.arange(m)[None, :]
    ainv = 0j if a64 == 0 else 1.0 / a64
    with np.errstate(all="ignore"):
        core = np.power(ainv, i) * np.power(w64, i * k) if n else np.zeros((0, m), complex)
    if a64 == 0 and n:
        core[0, :] = 1.0  # 0^0: apow starts at (1, 0)
    terms = x.astype(np.float64)[:, :, None] * core[None, :, :]
    return terms.sum(axis=1), np.abs(terms).sum(axis=1)


MEASURED_WORST = 0.79  # the largest |err| / (n * eps32 * sum |term|) over the cases below (see the docstring)


def _worst_ratio():
    eps = float(np.finfo(np.float32).eps)
    worst = 0.0
    for name in FINITE_SETS:
        for n, m in [(1, 1), (16, 16), (100, 37), (37, 100), (256, 256)]:
            w, a = so.param_sets(m)[name]
            x = seeded(12000 + n + m).uniform(-1, 1, (2, n)).astype(np.float32)
            want, mag = _f64_czt(x, m, w, a)
            err = np.abs(so.czt(x, m, w, a).astype(np.complex128) - want)
            worst = max(worst, float(np.max(err / (n * eps * mag + 1e-300))))
    return worst


def test_czt_oracle_agrees_with_float64():
    """The oracle (not the device) against float64 at n, m <= 256 over the finite parameter sets: the worst
    |err| / (n * eps32 * sum |term|) measured is 0.79 (seeds 12000 + n + m); four times that is asserted, as margin for other seeds.
    (The f32 recurrences of wnk and apow lose about one ulp per step, hence an error that grows with n.)"""
    worst = _worst_ratio()
    print(f"worst ratio {worst:.4f}")
    assert worst <= 4 * MEASURED_WORST, worst


def test_czt_as_dft_agrees_with_numpy_fft():
    eps = float(np.finfo(np.float32).eps)
    for n in (1, 8, 100, 256):
        x = seeded(12100 + n).uniform(-1, 1, (2, n)).astype(np.float32)
        w, a = so.param_sets(n)["dft"]
        got = so.czt(x, n, w, a).astype(np.complex128)
        want = np.fft.fft(x.astype(np.float64), axis=1)
        mag = np.abs(x.astype(np.float64)).sum(axis=1, keepdims=True)
        assert np.all(np.abs(got - want) <= 4 * MEASURED_WORST * n * eps * mag), n  # the bound of the float64 check: |term| = |x[i]| here


# ---- the C ABI's argument checks ----------------------------------------------------------------------------------------------------------
def test_argument_checks_in_order_with_a_null_context(hiplib):
    """include/kofft_hip.h, every error in its order, host and kofft_hip_dev_* forms -- no context needed."""
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    for fn in (hiplib.kofft_hip_czt_f32, hiplib.kofft_hip_dev_czt_f32):
        args = (1.0, 0.0, 1.0, 0.0)
        assert fn(None, None, None, 5000, 5000, *args, 0) == 0  # batch == 0 before everything
        assert fn(None, None, None, 5000, 0, *args, 3) == 0     # m == 0
        assert fn(None, p, p, 4097, 4, *args, 1) == -2          # the bounds
        assert fn(None, p, p, 4, 4097, *args, 1) == -2
        assert fn(None, p, p, 4096, 4096, *args, 1) == -3       # then the null context
        assert fn(None, p, p, 0, 4, *args, 1) == -3
    for fn in (hiplib.kofft_hip_goertzel_f32, hiplib.kofft_hip_dev_goertzel_f32):
        assert fn(None, None, None, 0, 0, C.c_float(0.0), None, 5000) == 0  # batch == 0
        assert fn(None, p, p, 0, 1, C.c_float(0.0), p, 1) == 1              # EMPTY_INPUT before the rate
        assert fn(None, p, p, 4, 1, C.c_float(0.0), p, 1) == 6              # INVALID_VALUE
        assert fn(None, p, p, 4, 1, C.c_float(-1.0), p, 1) == 6
        assert fn(None, None, None, 4, 1, C.c_float(1.0), None, 0) == 0     # no frequencies
        assert fn(None, p, p, (1 << 26) + 1, 1, C.c_float(1.0), p, 1) == -2
        assert fn(None, p, p, 4, 1, C.c_float(1.0), p, 1025) == -2
        assert fn(None, p, p, 4, 1, C.c_float(1.0), p, 1) == -3
        assert fn(None, p, p, 4, 1, C.c_float(float("nan")), p, 1) == -3    # a NaN rate passes the comparison
    assert hiplib.kofft_hip_set_czt_route(None, 0) == -3
    t = hiplib.kofft_hip_czt_table_f32
    assert t(0, 4, 1.0, 0.0, 1.0, 0.0, None) == 0 and t(4, 0, 1.0, 0.0, 1.0, 0.0, None) == 0
    assert t(4097, 4, 1.0, 0.0, 1.0, 0.0, p) == -2 and t(4, 4, 1.0, 0.0, 1.0, 0.0, None) == -3
    g = hiplib.kofft_hip_goertzel_coeff_f32
    assert g(0, C.c_float(1.0), p, 1, p) == 1 and g(4, C.c_float(0.0), p, 1, p) == 6 and g(4, C.c_float(1.0), None, 0, None) == 0
    assert g(4, C.c_float(1.0), p, 1025, p) == -2 and g(4, C.c_float(1.0), None, 1, p) == -3 and g(4, C.c_float(1.0), p, 1, None) == -3


# ---- machine code ---------------------------------------------------------------------------------------------------------------------------
LIB = ROOT / "kofft_amd" / "lib" / "libkofft_hip.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")


@pytest.mark.skipif(not LIB.exists() or not (LLVM / "llvm-objdump").exists(), reason="needs the built library and ROCm's llvm-objdump")
def test_spectral_kernels_have_no_fused_instruction_and_the_direct_kernels_stay_six():
    """-ffp-contract=off and the kernels' own arithmetic: czt.rs and goertzel.rs do not fuse.  (The square root is the called device
    function spectral_root_cr, a function of its own in the listing: its correctly rounded expansion holds fused operations.)"""
    sys.path.insert(0, str(ROOT / "tools"))
    from check_store_hazard import disassemble
    from test_trig_direct_cpu import _functions

    mine, direct = {}, set()
    for _, listing in disassemble(LIB):
        for func, lines in _functions(listing):
            if "czt_recur_kernel" in func or "goertzel_kernel" in func:
                mine[func] = lines
            if "direct_tiled_kernel" in func or "direct_simple_kernel" in func:
                direct.add(func)
    assert len(direct) == 6, sorted(direct)
    assert sum("czt_recur_kernel" in f for f in mine) == 2 and sum("goertzel_kernel" in f for f in mine) == 1, sorted(mine)
    bad = re.compile(r"^\s*(v_fma\w*|v_pk_fma\w*|v_fmac\w*|v_mac_\w*|v_mad_f32|v_mad_legacy\w*|v_mfma\w*|v_dot\w*)\b")
    for func, lines in mine.items():
        hits = [ln for ln in lines if bad.match(ln)]
        assert not hits, f"{func}: {hits[:3]}"
        assert any(re.match(r"^\s*v_(pk_)?mul_f32", ln) for ln in lines), func


# ---- sanitizers on the new host code -----------------------------------------------------------------------------------------------------------
def test_spectral_tables_under_asan_ubsan(tmp_path):
    exe = tmp_path / "sanitize_spectral_tables"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-ffp-contract=off"]
    subprocess.run(["g++", "-std=c++17", *flags, str(ROOT / "tests" / "cpp" / "sanitize_spectral_tables.cpp"),
                    str(ROOT / "kofft_amd" / "csrc" / "tables.cpp"), "-lm", "-pthread", "-o", str(exe)], check=True, capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert res.returncode == 0, res.stdout + res.stderr
    assert "0 problems" in res.stdout
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
