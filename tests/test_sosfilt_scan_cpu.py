"""IIR filtering of rows as a scan along time without a GPU: properties of the test oracle
(tests/sosfilt_scan_oracle.py: one chunk is the sequential oracle, the first chunk always is, reverse is flip), the oracle against
scipy.signal.sosfilt in float64 under twice the error measured for every (design, chunk) case, the sosfiltfilt composition through the
scan likewise, the C entries' argument checks in the header's order with a null context, the chunk query, the Python errors before any
context, and the scan functions of sosfilt_plan.h against an enumeration in a stand-alone program under AddressSanitizer +
UndefinedBehaviorSanitizer."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sosfilt_oracle as so
import sosfilt_scan_oracle as sc

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
VP = C.c_void_p
OK, EMPTY, MISMATCH, INVALID, UNSUPPORTED, NULL = 0, 1, 3, 6, -2, -3

# E = max|y - scipy float64| / max|scipy float64| on _accuracy_case's data: 2 rows of a 440 Hz sine at 48 kHz plus noise of 0.1 plus an
# offset of 0.1.  The recommended chunks, 1024 and 4096, run on 2^21 + 777 samples (2049 and 513 seams: the size at which seam roundings
# accumulate), chunk 256 on 2^18 + 777 samples (1027 seams).  E_scan: the scan oracle, measured on the CPU with the committed oracle,
# asserted at twice the value (the data are seeded: the margin covers other libm builds and other seeds' neighbourhood, nothing more).
# E_seq: the sequential filter (scipy.signal.sosfilt on float32, which is tests/sosfilt_oracle.py bit for bit) on the same data, reported
# and not asserted.  Poles within ~1e-3 of the unit circle cut into chunks of 256 cost a factor 3 to 4: a seam's rounding lives for
# thousands of samples there, which is why kofft_hip_sosfilt_scan_chunk never names less than 1024.
SMALL, LARGE = 18, 21  # log2 of the samples a row, less the 777
SIZE_OF_CHUNK = {256: SMALL, 1024: LARGE, 4096: LARGE}
#   (design, chunk): E_scan
ACCURACY_MEASURED = {
    ("butter4_low_0.002", 256): 2.442e-3, ("butter4_low_0.002", 1024): 7.432e-4, ("butter4_low_0.002", 4096): 7.426e-4,
    ("butter2_high_0.001", 256): 9.466e-4, ("butter2_high_0.001", 1024): 3.972e-4, ("butter2_high_0.001", 4096): 4.139e-4,
    ("ellip8_0.05", 256): 2.092e-5, ("ellip8_0.05", 1024): 2.163e-5, ("ellip8_0.05", 4096): 2.150e-5,
    ("butter8_band_0.2_0.5", 256): 1.398e-5, ("butter8_band_0.2_0.5", 1024): 1.302e-5, ("butter8_band_0.2_0.5", 4096): 1.302e-5,
    ("butter8_band_0.01_0.02", 256): 7.481e-5, ("butter8_band_0.01_0.02", 1024): 7.925e-5, ("butter8_band_0.01_0.02", 4096): 7.689e-5,
}
#   (design, size): E_seq
E_SEQ_MEASURED = {("butter4_low_0.002", SMALL): 5.955e-4, ("butter2_high_0.001", SMALL): 3.558e-4, ("ellip8_0.05", SMALL): 1.871e-5,
                  ("butter8_band_0.2_0.5", SMALL): 1.406e-5, ("butter8_band_0.01_0.02", SMALL): 6.419e-5,
                  ("butter4_low_0.002", LARGE): 7.839e-4, ("butter2_high_0.001", LARGE): 4.760e-4, ("ellip8_0.05", LARGE): 2.128e-5,
                  ("butter8_band_0.2_0.5", LARGE): 1.302e-5, ("butter8_band_0.01_0.02", LARGE): 8.067e-5}
# the cases the GPU test runs on the device as well: chunk 256 at the small size, and one at the full size
GPU_CASES = [k for k in sorted(ACCURACY_MEASURED) if k[1] == 256] + [("butter2_high_0.001", 1024)]

# sosfiltfilt(chunk=...) against scipy.signal.sosfiltfilt in float64 on _filtfilt_case's data, chunks 64 and 1024: the worst measured
# value (ellip8, chunk 1024), asserted at twice that; the sequential composition measures 2.23e-5 on the same data (DESIGN 5.29 has
# 2.2e-5 on its own, asserted at 4.4e-5).
FILTFILT_SCAN_MEASURED = 2.51e-5
FILTFILT_CASES = ["butter4_low", "butter8_band", "ellip8"]


@pytest.fixture(autouse=True, scope="module")
def _the_library_has_the_scan(hiplib):
    for name in ("kofft_hip_sosfilt_scan_f32", "kofft_hip_dev_sosfilt_scan_f32", "kofft_hip_sosfilt_scan_chunk"):
        assert hasattr(hiplib, name), f"{name} is not exported"
    from kofft_amd import iir

    assert hasattr(iir, "sosfilt_scan") and hasattr(iir, "scan_chunk")


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def rel_err(got, want64):
    return float(np.max(np.abs(np.asarray(got, np.float64) - want64)) / np.max(np.abs(want64)))


def table_designs():
    from scipy import signal

    d = {
        "butter4_low_0.002": signal.butter(4, 0.002, "low", output="sos"),
        "butter2_high_0.001": signal.butter(2, 0.001, "high", output="sos"),  # a DC blocker
        "ellip8_0.05": signal.ellip(8, 0.1, 80, 0.05, output="sos"),
        "butter8_band_0.2_0.5": signal.butter(8, [0.2, 0.5], "band", output="sos"),
        "butter8_band_0.01_0.02": signal.butter(8, [0.01, 0.02], "band", output="sos"),
    }
    return {k: np.ascontiguousarray(v, F) for k, v in d.items()}


def _signal(rows, nx, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(nx)
    return (np.sin(2 * np.pi * 440.0 / 48000.0 * t)[None, :] + 0.1 * rng.standard_normal((rows, nx)) + 0.1).astype(F)


@functools.lru_cache(maxsize=None)
def _accuracy_case(name, chunk):
    """(sos, x, scipy.signal.sosfilt in float64 on the float32 inputs and coefficients) at the size of the chunk's cases: computed once
    per design and size, shared, never written."""
    return _accuracy_data(name, SIZE_OF_CHUNK[chunk])


@functools.lru_cache(maxsize=None)
def _accuracy_data(name, log2):
    from scipy import signal

    sos = table_designs()[name]
    x = _signal(2, (1 << log2) + 777, 30000)
    want = signal.sosfilt(sos.astype(np.float64), x.astype(np.float64), axis=-1)
    for a in (sos, x, want):
        a.setflags(write=False)
    return sos, x, want


def _filtfilt_case(name):
    return so.designs()[name], _signal(3, 5000, 30001)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("sections", [1, 3, 8, 9, 17])
def test_one_chunk_is_the_sequential_oracle(sections, reverse):
    sos = so.cascade(sections)
    rng = np.random.default_rng(30800 + sections)
    x = rng.uniform(-1, 1, (3, 100)).astype(F)
    zi = rng.uniform(-1, 1, (3, sections, 2)).astype(F)
    want = so.sosfilt_ref(sos, x, zi, reverse)
    for chunk in (128, 4096):
        got = sc.sosfilt_scan_ref(sos, x, chunk, zi, reverse)
        assert _same(got[0], want[0]) and _same(got[1], want[1])
    y, zf = sc.sosfilt_scan_ref(sos, x[0], 128, zi[0], reverse)
    assert _same(y, want[0][0]) and _same(zf, want[1][0])


@pytest.mark.parametrize("chunk", [32, 64, 96])
def test_the_first_chunk_is_the_sequential_oracles(chunk):
    sos = so.cascade(10)
    rng = np.random.default_rng(30900)
    x = rng.uniform(-1, 1, (3, 500)).astype(F)
    zi = rng.uniform(-1, 1, (3, 10, 2)).astype(F)
    assert _same(sc.sosfilt_scan_ref(sos, x, chunk, zi)[0][:, :chunk], so.sosfilt_ref(sos, x, zi)[0][:, :chunk])
    assert _same(sc.sosfilt_scan_ref(sos, x, chunk, zi, True)[0][:, -chunk:], so.sosfilt_ref(sos, x, zi, True)[0][:, -chunk:])


@pytest.mark.parametrize("name", ["butter5_band", "ellip8"])
def test_reverse_equals_flip(name):
    sos = so.designs()[name]
    rng = np.random.default_rng(30950)
    x = rng.uniform(-1, 1, (5, 333)).astype(F)
    zi = rng.uniform(-1, 1, (5, sos.shape[0], 2)).astype(F)
    y, zf = sc.sosfilt_scan_ref(sos, x, 64, zi, reverse=True)
    yf, zff = sc.sosfilt_scan_ref(sos, x[:, ::-1], 64, zi)
    assert _same(y, np.ascontiguousarray(yf[:, ::-1])) and _same(zf, zff)


def test_the_transition_matrix_is_block_lower_triangular_and_the_carry_leaves_the_zeros_out():
    """M's columns of the sections behind component i's are exact zeros; an Inf in the last section's state stays there."""
    sos = so.cascade(4)
    M = sc.transition(sos, 32)
    assert M.shape == (8, 8) and M.dtype == F
    for i in range(8):
        assert not M[i, 2 * (i // 2) + 2:].any()
    z0 = np.ones((1, 8), F)
    z0[0, 6] = np.inf
    Z = sc.carry(M, z0, np.zeros((1, 3, 8), F))
    assert np.isfinite(Z[0, :, :6]).all() and not np.isfinite(Z[0, 1:, 6:]).all()


def test_pins_by_hand():
    """One section b = (1, 2, 3), a = (1, 0.5, 0.25) has the one-step matrix [[-0.5, 1], [-0.25, 0]] (y = z0: z0' = -(0.5 y) + z1,
    z1' = -(0.25 y)); M of a chunk is its power, and the seam state is M Z + p in that order of sums."""
    sos = np.array([[1, 2, 3, 1, 0.5, 0.25]], F)
    A = np.array([[-0.5, 1], [-0.25, 0]], np.float64)
    M = sc.transition(sos, 32)
    assert np.allclose(M, np.linalg.matrix_power(A, 32), rtol=1e-5, atol=1e-12)
    x = np.arange(70, dtype=F) / 8
    zi = np.array([[0.5, -2.0]], F)
    _, p = so.sosfilt_ref(sos, x[:32])
    y, zf = sc.sosfilt_scan_ref(sos, x, 32, zi)
    z1 = np.array([(M[0, 0] * zi[0, 0] + M[0, 1] * zi[0, 1]) + p[0, 0], (M[1, 0] * zi[0, 0] + M[1, 1] * zi[0, 1]) + p[0, 1]], F)
    assert _same(y[32:64], so.sosfilt_ref(sos, x[32:64], z1[None, :])[0])


@pytest.mark.parametrize("name,chunk", sorted(ACCURACY_MEASURED))
def test_the_oracle_against_scipy_float64(name, chunk):
    sos, x, want = _accuracy_case(name, chunk)
    got, _ = sc.sosfilt_scan_ref(sos, x, chunk)
    e = rel_err(got, want)
    print(f"{name} sections={sos.shape[0]} chunk={chunk}: E_scan = {e:.3e} (measured {ACCURACY_MEASURED[name, chunk]:.3e}), E_seq = "
          f"{E_SEQ_MEASURED[name, SIZE_OF_CHUNK[chunk]]:.3e} on {x.shape[1]} samples a row")
    assert e <= 2 * ACCURACY_MEASURED[name, chunk]


@pytest.mark.parametrize("name", FILTFILT_CASES)
def test_sosfiltfilt_through_the_scan_against_scipy_float64(name):
    from scipy import signal

    sos, x = _filtfilt_case(name)
    want = signal.sosfiltfilt(sos.astype(np.float64), x.astype(np.float64), axis=-1)
    for chunk in (64, 1024):
        got = sc.sosfiltfilt_scan_ref(sos, x, chunk)
        assert got.dtype == F and got.shape == x.shape
        e = rel_err(got, want)
        print(f"{name} chunk={chunk}: max|d| / max|y| = {e:.3e}")
        assert e <= 2 * FILTFILT_SCAN_MEASURED, (name, chunk, e)
    # one chunk over the padded row: the sequential composition's bytes
    assert _same(sc.sosfiltfilt_scan_ref(sos, x, 8192), so.sosfiltfilt_ref(sos, x))


@pytest.mark.parametrize("name", ["kofft_hip_sosfilt_scan_f32", "kofft_hip_dev_sosfilt_scan_f32"])
def test_argument_checks_in_the_headers_order_with_a_null_context(hiplib, name):
    """(ctx, x, rows, nx, sos, sections, zi, zf, chunk, flags, out): each line violates one check and every later one it can."""
    buf = np.zeros(64, F)
    p, null = VP(buf.ctypes.data), VP(None)
    call = lambda *a: getattr(hiplib, name)(null, *a)  # noqa: E731
    assert call(null, 0, 5, null, 0, null, null, 0, 6, null) == OK              # 1: no rows, whatever else
    assert call(null, 5, 0, null, 0, null, p, 33, 6, null) == OK                # 1: no samples
    assert not buf.any()                                                         #    zf is not written either
    assert call(null, 2, 4, null, 0, null, null, 0, 6, null) == EMPTY           # 2: no sections, before the flags
    assert call(null, 1 << 62, 4, null, 1, null, null, 0, 2, null) == INVALID   # 3: an unknown flag bit, before the chunk
    assert call(null, 1 << 62, 4, null, 1, null, null, 0, 1, null) == INVALID   # 3a: chunk 0, before the byte counts
    assert call(null, 1 << 62, 4, null, 1, null, null, 33, 0, null) == INVALID  # 3a: no multiple of the tile
    assert call(null, 1 << 62, 4, null, 1, null, null, 48, 0, null) == INVALID
    assert call(null, 1 << 62, 4, null, 1, null, null, 32, 1, null) == UNSUPPORTED  # 4: rows * nx * 4
    assert call(null, 1 << 40, 1, null, 1 << 40, null, null, 32, 0, null) == UNSUPPORTED  # 4: rows * sections * 8
    assert call(null, 1, 1, null, 1 << 62, null, null, 32, 0, null) == UNSUPPORTED  # 4: sections * 24
    assert call(null, 2, 4, p, 1, null, null, 32, 0, p) == NULL                  # 5: x
    assert call(p, 2, 4, null, 1, null, null, 32, 0, p) == NULL                  # 5: sos
    assert call(p, 2, 4, p, 1, null, null, 32, 0, null) == NULL                  # 5: out
    assert call(p, 2, 4, p, 1, p, p, 64, 1, p) == NULL                           # 5: the context, before every overlap


def test_overlap_and_a0_checks(hiplib):
    buf = np.zeros(256, F)
    base = buf.ctypes.data
    at = lambda i: VP(base + 4 * i)  # noqa: E731
    fake = VP(base + 4 * 200)  # (never touched: every call below fails a check first)
    sos_ok = np.array([[1, 0, 0, 1, 0, 0]], F)
    s = VP(sos_ok.ctypes.data)
    for name in ("kofft_hip_sosfilt_scan_f32", "kofft_hip_dev_sosfilt_scan_f32"):
        call = lambda *a: getattr(hiplib, name)(fake, *a)  # noqa: E731
        assert call(at(0), 2, 4, s, 1, None, None, 32, 0, at(4)) == INVALID        # 6: out over x, not exactly
        assert call(at(0), 2, 4, s, 1, at(40), at(42), 32, 0, at(16)) == INVALID   # 6: zf over zi, not exactly
        assert call(at(0), 2, 4, at(20), 1, None, None, 32, 0, at(16)) == INVALID  # 7: out over sos
        assert call(at(0), 2, 4, s, 1, None, at(20), 32, 0, at(16)) == INVALID     # 7: zf over out
        assert call(at(0), 2, 4, s, 1, None, at(6), 32, 0, at(16)) == INVALID      # 7: zf over x
        assert call(at(0), 2, 4, s, 1, at(18), None, 32, 0, at(16)) == INVALID     # 7: out over zi
    bad = np.array([[1, 0, 0, 1, 0, 0], [1, 0, 0, 2, 0, 0]], F)
    assert hiplib.kofft_hip_sosfilt_scan_f32(fake, at(0), 2, 4, VP(bad.ctypes.data), 2, None, None, 32, 0, at(16)) == INVALID  # 8: a0
    assert not buf.any()


def test_chunk_query(hiplib):
    """kofft_hip_sosfilt_scan_chunk: a multiple of the tile, never below 1024; the measured rule of DESIGN 5.30."""
    from kofft_amd import iir

    k = C.c_size_t(7)
    assert hiplib.kofft_hip_sosfilt_scan_chunk(1, 1000, 1, None) == NULL
    assert hiplib.kofft_hip_sosfilt_scan_chunk(0, 0, 0, C.byref(k)) == OK and k.value >= 1024
    for rows in (1, 2, 15, 16, 64, 4096, 65536):
        for nx in (1, 3000, 48000, 1 << 20, 28_800_000, 1 << 24):
            for sections in (1, 4, 8, 12):
                got = iir.scan_chunk(rows, nx, sections)
                assert got >= 1024 and got % 32 == 0, (rows, nx, sections, got)
    # the rule read off profiles/sosfilt_scan_bench.txt: 1024 below 2^22 samples a row, 2048 from there on, 4096 for one such row through
    # eight sections or more
    assert [iir.scan_chunk(r, n, s) for r, n, s in [(64, 1 << 20, 12), (4096, 48000, 1), (65536, 3000, 8), (1, (1 << 22) - 1, 8)]] == [1024] * 4
    assert [iir.scan_chunk(r, n, s) for r, n, s in [(16, 1 << 24, 1), (16, 1 << 24, 12), (1, 28_800_000, 4), (2, 1 << 22, 8)]] == [2048] * 4
    assert [iir.scan_chunk(1, 28_800_000, s) for s in (7, 8, 12)] == [2048, 4096, 4096]
    with pytest.raises(ValueError):
        iir.scan_chunk(-1, 5, 1)


def test_python_errors_before_any_device():
    import kofft_amd
    from kofft_amd import iir

    before = iir._default
    E = kofft_amd.FftError
    x = np.ones((2, 50), F)
    sos = so.cascade(2)
    bad_a0 = sos.copy()
    bad_a0[1, 3] = 0.5
    for fn, args, kw, code in [(iir.sosfilt_scan, (np.ones((0, 6), F), x), {}, EMPTY), (iir.sosfilt_scan, (bad_a0, x), {}, INVALID),
                               (iir.sosfilt_scan, (sos, x), {"chunk": 0}, INVALID), (iir.sosfilt_scan, (sos, x), {"chunk": 33}, INVALID),
                               (iir.sosfilt_scan, (sos, x), {"chunk": -32}, INVALID), (iir.sosfiltfilt, (sos, x), {"chunk": 48}, INVALID),
                               (iir.sosfiltfilt, (sos, x), {"chunk": 0}, INVALID),
                               (iir.sosfilt_scan, (sos, x, np.zeros((2, 3, 2), F)), {"chunk": 32}, MISMATCH),
                               (iir.sosfilt_scan, (sos, x[0], np.zeros((2, 2, 2), F)), {}, MISMATCH)]:
        with pytest.raises(E) as e:
            fn(*args, **kw)
        assert e.value.code == code, (fn.__name__, kw, code)
    for args in [(np.ones((2, 5), F), x), (sos, np.ones((2, 3, 4), F))]:
        with pytest.raises(TypeError):
            iir.sosfilt_scan(*args)
    assert iir.sosfilt_scan(sos, np.ones((0, 50), F)).shape == (0, 50) and iir.sosfilt_scan(sos, np.ones((2, 0), F), chunk=64).shape == (2, 0)
    zi = np.ones((2, 2, 2), F)
    y, zf = iir.sosfilt_scan(sos, np.ones((2, 0), F), zi)
    assert y.shape == (2, 0) and _same(zf, zi) and zf is not zi
    assert iir._default is before, "a context was created before the errors"


def test_the_scan_plan_arithmetic_under_asan_ubsan(tmp_path):
    """The scan functions of sosfilt_plan.h against an enumeration of every sample of every chunk of both walks, both directions, in a
    stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer."""
    exe = tmp_path / "sanitize_sosfilt_scan_plan"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", *flags, str(ROOT / "tests" / "cpp" / "sanitize_sosfilt_scan_plan.cpp"), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 problems" in res.stdout
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
