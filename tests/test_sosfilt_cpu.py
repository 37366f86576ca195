"""IIR filtering of rows without a GPU: the test oracle (tests/sosfilt_oracle.py) against scipy.signal.sosfilt on
float32 arrays bit for bit (outputs and final states), reverse against flip, the steady state against scipy.signal.sosfilt_zi, the
sosfiltfilt composition against scipy in float64 under twice the margin measured on this data, pins by hand, the C
entries' argument checks in the header's order with a null context, the Python errors before any context, and sosfilt_plan.h against
an enumeration in a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sosfilt_oracle as so

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
VP = C.c_void_p
OK, EMPTY, MISMATCH, INVALID, UNSUPPORTED, NULL = 0, 1, 3, 6, -2, -3

# The worst max|oracle - scipy float64| / max|scipy float64| of sosfiltfilt_ref over FILTFILT_CASES, measured on the CPU (2.2e-5, at
# ellip8: poles within 0.01 of the unit circle amplify the float32 rounding of the recurrence); the assertion is twice that.  The data
# are seeded, so the margin only covers other libm builds.
FILTFILT_MEASURED = 2.2e-5
FILTFILT_CASES = ["butter2_low", "butter4_high", "butter5_band", "butter6_low", "butter8_band", "ellip8"]


@pytest.fixture(autouse=True, scope="module")
def _the_library_has_the_filter(hiplib):
    """Every test here pins kofft_hip_sosfilt_f32's definition or its host side: without the entry points none of them means anything."""
    for name in ("kofft_hip_sosfilt_f32", "kofft_hip_dev_sosfilt_f32", "kofft_hip_set_sosfilt_tiled", "kofft_hip_sosfilt_route"):
        assert hasattr(hiplib, name), f"{name} is not exported"
    from kofft_amd import iir  # noqa: F401


def _scipy(sos, x, zi_rows=None):
    """scipy.signal.sosfilt on float32 arrays: (y, zf [rows, sections, 2])."""
    from scipy import signal

    rows, sections = x.shape[0], sos.shape[0]
    zi = np.zeros((sections, rows, 2), F) if zi_rows is None else np.ascontiguousarray(zi_rows.transpose(1, 0, 2))
    y, zf = signal.sosfilt(sos, x, axis=-1, zi=zi)
    assert y.dtype == F and zf.dtype == F
    return y, np.ascontiguousarray(zf.transpose(1, 0, 2))


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_nan(a, b):
    """bit for bit, a NaN against a NaN whatever its sign and payload"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and (na == nb).all() and a[~na].tobytes() == b[~nb].tobytes()


DESIGNS = sorted(so.designs())


@pytest.mark.parametrize("name", DESIGNS)
def test_oracle_equals_scipy_sosfilt_bit_for_bit(name):
    sos = so.designs()[name]
    rng = np.random.default_rng(29100 + len(name) + sos.shape[0])
    x = rng.uniform(-1, 1, (7, 1000)).astype(F)
    zi = rng.uniform(-1, 1, (7, sos.shape[0], 2)).astype(F)
    for state in (None, zi):
        want_y, want_z = _scipy(sos, x, state)
        got_y, got_z = so.sosfilt_ref(sos, x, state)
        assert _same(got_y, want_y), f"{name}: outputs"
        assert _same(got_z, want_z), f"{name}: final states"


@pytest.mark.parametrize("name", ["butter4_low", "ellip8"])
def test_oracle_equals_scipy_on_nan_and_inf(name):
    sos = so.designs()[name]
    x = np.random.default_rng(29150).uniform(-1, 1, (3, 400)).astype(F)
    x[0, 100] = np.nan
    x[1, 50] = np.inf
    want_y, want_z = _scipy(sos, x)
    got_y, got_z = so.sosfilt_ref(sos, x)
    assert np.isnan(want_y[0, 100:]).all() and np.isfinite(want_y[0, :100]).all() and np.isfinite(want_y[2]).all()
    assert not np.isfinite(want_y[1, 50:]).any()
    assert _same_nan(got_y, want_y) and _same_nan(got_z, want_z)


def test_oracle_equals_scipy_through_the_subnormal_decay_tail():
    """An impulse and 5999 zeros through a Butterworth low-pass: the tail decays through the float32 subnormals to zero."""
    sos = so.designs()["butter4_low"]
    x = np.zeros((1, 6000), F)
    x[0, 0] = 1
    want_y, want_z = _scipy(sos, x)
    tiny = np.finfo(F).tiny
    sub = (want_y != 0) & (np.abs(want_y) < tiny)
    assert sub.sum() > 100, "the expected output holds subnormals"
    got_y, got_z = so.sosfilt_ref(sos, x)
    assert _same(got_y, want_y) and _same(got_z, want_z)


@pytest.mark.parametrize("name", ["butter5_band", "ellip8"])
def test_reverse_equals_flip(name):
    sos = so.designs()[name]
    rng = np.random.default_rng(29200)
    x = rng.uniform(-1, 1, (5, 333)).astype(F)
    zi = rng.uniform(-1, 1, (5, sos.shape[0], 2)).astype(F)
    y, zf = so.sosfilt_ref(sos, x, zi, reverse=True)
    yf, zff = so.sosfilt_ref(sos, x[:, ::-1], zi)
    assert _same(y, np.ascontiguousarray(yf[:, ::-1])) and _same(zf, zff)


@pytest.mark.parametrize("name", DESIGNS)
def test_sosfilt_zi_against_scipy(name):
    from scipy import signal

    from kofft_amd import iir

    sos = so.designs()[name].astype(np.float64)
    want = signal.sosfilt_zi(sos).astype(F)
    # (the same float32 values: behind a high-pass section the step's steady state is 0, and the sign of a zero is the solver's)
    assert np.array_equal(iir.sosfilt_zi(sos).astype(F), want)
    assert np.array_equal(so.sosfilt_zi_ref(sos).astype(F), want)
    assert iir.default_padlen(sos) == so.default_padlen(sos)


def _filtfilt_case(name):
    sos = so.designs()[name]
    x = np.random.default_rng(29300 + sos.shape[0]).uniform(-1, 1, (3, 700)).astype(F)
    return sos, x


@pytest.mark.parametrize("name", FILTFILT_CASES)
def test_sosfiltfilt_composition_against_scipy_float64(name):
    from scipy import signal

    sos, x = _filtfilt_case(name)
    want = signal.sosfiltfilt(sos.astype(np.float64), x.astype(np.float64), axis=-1)
    got = so.sosfiltfilt_ref(sos, x)
    assert got.dtype == F and got.shape == x.shape
    rel = float(np.max(np.abs(got.astype(np.float64) - want)) / np.max(np.abs(want)))
    print(f"{name}: max|d| / max|y| = {rel:.3e}")
    assert rel <= 2 * FILTFILT_MEASURED, (name, rel)
    # padlen given, and none
    for padlen in (0, 5):
        want = signal.sosfiltfilt(sos.astype(np.float64), x.astype(np.float64), axis=-1, padlen=padlen)
        got = so.sosfiltfilt_ref(sos, x, padlen)
        assert float(np.max(np.abs(got - want)) / np.max(np.abs(want))) <= 2 * FILTFILT_MEASURED, (name, padlen)


def test_default_padlen_is_scipys():
    """scipy raises for an input no longer than its padlen: the longest refused length is the padlen."""
    from scipy import signal

    for name in ("butter2_low", "butter5_low", "butter5_band", "ellip8"):
        sos = so.designs()[name].astype(np.float64)
        edge = so.default_padlen(sos)
        with pytest.raises(ValueError):
            signal.sosfiltfilt(sos, np.ones(edge))
        signal.sosfiltfilt(sos, np.ones(edge + 1))


def test_pins_by_hand():
    """One section, three samples: b = (1, 2, 3), a = (1, 0.5, 0.25), zero state.
    t=0: y = 1, z0 = (2 - 0.5) + 0 = 1.5, z1 = 3 - 0.25 = 2.75;  t=1: x = 2: y = 2 + 1.5 = 3.5, z0 = (4 - 1.75) + 2.75 = 5,
    z1 = 6 - 0.875 = 5.125;  t=2: x = -1: y = -1 + 5 = 4, z0 = (-2 - 2) + 5.125 = 1.125, z1 = -3 - 1 = -4."""
    sos = np.array([[1, 2, 3, 1, 0.5, 0.25]], F)
    y, zf = so.sosfilt_ref(sos, np.array([1, 2, -1], F))
    assert y.tolist() == [1.0, 3.5, 4.0] and zf.tolist() == [[1.125, -4.0]]
    # the same samples walked from the end: the filter of (-1, 2, 1), flipped back
    # t=2: x = -1: y = -1, z0 = (-2 + 0.5) = -1.5, z1 = -3 + 0.25 = -2.75;  t=1: x = 2: y = 2 - 1.5 = 0.5, z0 = (4 - 0.25) - 2.75 = 1,
    # z1 = 6 - 0.125 = 5.875;  t=0: x = 1: y = 1 + 1 = 2, z0 = (2 - 1) + 5.875 = 6.875, z1 = 3 - 0.5 = 2.5
    y, zf = so.sosfilt_ref(sos, np.array([1, 2, -1], F), reverse=True)
    assert y.tolist() == [2.0, 0.5, -1.0] and zf.tolist() == [[6.875, 2.5]]
    # a state: y0 = x0 + z0
    y, zf = so.sosfilt_ref(sos, np.array([1], F), np.array([[[10, 20]]], F))
    assert y.tolist() == [11.0] and zf.tolist() == [[(2 - 5.5) + 20, 3 - 2.75]]
    # two sections are the composition of one and one
    two = np.array([[1, 2, 3, 1, 0.5, 0.25], [0.5, -1, 0.25, 1, -0.5, 0.125]], F)
    x = np.array([1, 2, -1, 4], F)
    y1, _ = so.sosfilt_ref(two[:1], x)
    y2, _ = so.sosfilt_ref(two[1:], y1)
    assert _same(so.sosfilt_ref(two, x)[0], y2)


def _call(hiplib, name, ctx, x, rows, nx, sos, sections, zi, zf, flags, out):
    return getattr(hiplib, name)(ctx, x, rows, nx, sos, sections, zi, zf, flags, out)


@pytest.mark.parametrize("name", ["kofft_hip_sosfilt_f32", "kofft_hip_dev_sosfilt_f32"])
def test_argument_checks_in_the_headers_order_with_a_null_context(hiplib, name):
    """(ctx, x, rows, nx, sos, sections, zi, zf, flags, out): each line violates one check and every later one it can."""
    buf = np.zeros(64, F)
    p, null = VP(buf.ctypes.data), VP(None)
    call = lambda *a: _call(hiplib, name, null, *a)  # noqa: E731
    assert call(null, 0, 5, null, 0, null, null, 6, null) == OK              # 1: no rows, whatever else
    assert call(null, 5, 0, null, 0, null, p, 6, null) == OK                 # 1: no samples
    assert not buf.any()                                                      #    zf is not written either
    assert call(null, 2, 4, null, 0, null, null, 6, null) == EMPTY           # 2: no sections, before the flags
    assert call(null, 1 << 62, 4, null, 1, null, null, 2, null) == INVALID   # 3: an unknown flag bit, before the byte counts
    assert call(null, 2, 4, null, 1, null, null, 1 << 31, null) == INVALID
    assert call(null, 1 << 62, 4, null, 1, null, null, 1, null) == UNSUPPORTED  # 4: rows * nx * 4
    assert call(null, 1 << 40, 1, null, 1 << 40, null, null, 0, null) == UNSUPPORTED  # 4: rows * sections * 8
    assert call(null, 1, 1, null, 1 << 62, null, null, 0, null) == UNSUPPORTED  # 4: sections * 24
    assert call(null, 2, 4, p, 1, null, null, 0, p) == NULL                  # 5: x
    assert call(p, 2, 4, null, 1, null, null, 0, p) == NULL                  # 5: sos
    assert call(p, 2, 4, p, 1, null, null, 0, null) == NULL                  # 5: out
    assert call(p, 2, 4, p, 1, p, p, 1, p) == NULL                           # 5: the context, before every overlap


def test_overlap_and_a0_checks(hiplib):
    """The checks behind the null ones need a context that is never dereferenced before they fail: any non-null pointer."""
    buf = np.zeros(256, F)
    base = buf.ctypes.data
    at = lambda i: VP(base + 4 * i)  # noqa: E731
    fake = VP(base + 4 * 200)  # (never touched: every call below fails a check first)
    sos_ok = np.array([[1, 0, 0, 1, 0, 0]], F)
    s = VP(sos_ok.ctypes.data)
    for name in ("kofft_hip_sosfilt_f32", "kofft_hip_dev_sosfilt_f32"):
        call = lambda *a: _call(hiplib, name, fake, *a)  # noqa: E731
        # rows = 2, nx = 4: x and out are 8 floats, the state 4 floats
        assert call(at(0), 2, 4, s, 1, None, None, 0, at(4)) == INVALID        # 6: out over x, not exactly
        assert call(at(4), 2, 4, s, 1, None, None, 0, at(0)) == INVALID
        assert call(at(0), 2, 4, s, 1, at(40), at(42), 0, at(16)) == INVALID   # 6: zf over zi, not exactly
        assert call(at(0), 2, 4, at(20), 1, None, None, 0, at(16)) == INVALID  # 7: out over sos
        assert call(at(0), 2, 4, at(41), 1, None, at(40), 0, at(16)) == INVALID  # 7: zf over sos
        assert call(at(0), 2, 4, s, 1, None, at(20), 0, at(16)) == INVALID     # 7: zf over out
        assert call(at(0), 2, 4, s, 1, None, at(6), 0, at(16)) == INVALID      # 7: zf over x
        assert call(at(0), 2, 4, s, 1, at(18), None, 0, at(16)) == INVALID     # 7: out over zi
    bad = np.array([[1, 0, 0, 1, 0, 0], [1, 0, 0, 2, 0, 0]], F)
    assert _call(hiplib, "kofft_hip_sosfilt_f32", fake, at(0), 2, 4, VP(bad.ctypes.data), 2, None, None, 0, at(16)) == INVALID  # 8: a0
    bad[1, 3] = np.nan
    assert _call(hiplib, "kofft_hip_sosfilt_f32", fake, at(0), 2, 4, VP(bad.ctypes.data), 2, None, None, 0, at(0)) == INVALID
    assert not buf.any()
    assert hiplib.kofft_hip_set_sosfilt_tiled(None, 1) == NULL


def test_route_query(hiplib):
    """The measured rule: the tiled kernel from 16 rows on."""
    from kofft_amd import iir

    r = C.c_int(7)
    assert hiplib.kofft_hip_sosfilt_route(5, None) == NULL
    assert hiplib.kofft_hip_sosfilt_route(0, C.byref(r)) == OK and r.value == 0
    routes = [iir.route(rows) for rows in range(1, 200)]
    assert routes == [0] * 15 + [1] * 184
    assert iir.route(65536) == 1 and iir.route(1 << 20) == 1 and iir.route((1 << 64) - 1) == 1
    with pytest.raises(ValueError):
        iir.route(-1)


def test_python_errors_before_any_device():
    import kofft_amd
    from kofft_amd import iir

    before = iir._default
    E = kofft_amd.FftError
    x = np.ones((2, 50), F)
    sos = so.cascade(2)
    bad_a0 = sos.copy()
    bad_a0[1, 3] = 0.5
    for fn, args, code in [(iir.sosfilt, (np.ones((0, 6), F), x), EMPTY), (iir.sosfilt, (bad_a0, x), INVALID),
                           (iir.sosfiltfilt, (bad_a0, x), INVALID), (iir.sosfilt_zi, (bad_a0,), INVALID),
                           (iir.sosfilt, (sos, x, np.zeros((2, 3, 2), F)), MISMATCH), (iir.sosfilt, (sos, x, np.zeros((2, 2), F)), MISMATCH),
                           (iir.sosfilt, (sos, x[0], np.zeros((2, 2, 2), F)), MISMATCH)]:
        with pytest.raises(E) as e:
            fn(*args)
        assert e.value.code == code, (fn.__name__, code)
    for fn, args in [(iir.sosfilt, (np.ones((2, 5), F), x)), (iir.sosfilt, (np.ones(6, F), x)), (iir.sosfilt, (sos, np.ones((2, 3, 4), F))),
                     (iir.sosfiltfilt, (sos, np.ones((2, 3, 4), F))), (iir.sosfilt_zi, (np.ones((2, 5)),))]:
        with pytest.raises(TypeError):
            fn(*args)
    edge = iir.default_padlen(sos)
    assert edge == 15
    for args in [(sos, np.ones((2, edge), F)), (sos, x, -1), (sos, x, 50)]:
        with pytest.raises(ValueError):
            iir.sosfiltfilt(*args)
    # nothing to filter: no device
    assert iir.sosfilt(sos, np.ones((0, 50), F)).shape == (0, 50) and iir.sosfilt(sos, np.ones((2, 0), F)).shape == (2, 0)
    zi = np.ones((2, 2, 2), F)
    y, zf = iir.sosfilt(sos, np.ones((2, 0), F), zi)
    assert y.shape == (2, 0) and _same(zf, zi) and zf is not zi
    assert iir.sosfiltfilt(sos, np.ones((0, 50), F)).shape == (0, 50)
    assert iir._default is before, "a context was created before the errors"


def test_the_plan_arithmetic_under_asan_ubsan(tmp_path):
    """sosfilt_plan.h against an enumeration of every sample of every tile of every row group, both directions, in a stand-alone
    program under AddressSanitizer + UndefinedBehaviorSanitizer."""
    exe = tmp_path / "sanitize_sosfilt_plan"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", *flags, str(ROOT / "tests" / "cpp" / "sanitize_sosfilt_plan.cpp"), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 problems" in res.stdout
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
