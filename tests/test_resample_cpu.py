"""Polyphase resampling without a GPU: the test oracle (tests/resample_oracle.py) against scipy in float64 under
the forward error bound of its own summation, the tap design against scipy.signal.firwin, pins by hand, the C entry's argument checks
in the header's order with a null context, the Python errors before any context, the route query, and resample_plan.h against an
enumeration in a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import resample_oracle as ro

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
VP = C.c_void_p
OK, EMPTY, MISMATCH, INVALID, UNSUPPORTED, NULL = 0, 1, 3, 6, -2, -3
@pytest.fixture(autouse=True, scope="module")
def _the_library_has_the_resampler(hiplib):
    """Every test here pins kofft_hip_resample_f32's definition or its host side: without the entry points none of them means anything."""
    for name in ("kofft_hip_resample_f32", "kofft_hip_dev_resample_f32", "kofft_hip_resample_route", "kofft_hip_resample_taps_f32"):
        assert hasattr(hiplib, name), f"{name} is not exported"


_bound = ro.forward_bound  # (J + 2) 2^-24 sum |h_k x_i| per output


SHAPES = [(1, 1, 37, 5), (3, 2, 50, 31), (160, 441, 900, 8821), (2, 1, 33, 41), (1, 3, 100, 61), (7, 5, 64, 9), (5, 7, 3, 200)]


@pytest.mark.parametrize("up,down,nx,nh", SHAPES)
def test_oracle_against_scipy_upfirdn_float64(up, down, nx, nh):
    from scipy import signal

    rng = np.random.default_rng(27000 + up + nh)
    x = rng.uniform(-1, 1, nx).astype(F)
    h = rng.uniform(-1, 1, nh).astype(F)
    want = signal.upfirdn(h.astype(np.float64), x.astype(np.float64), up, down)
    out_len = ro.full_len(nx, nh, up, down)
    assert want.shape == (out_len,)
    got = ro.resample_ref(x, h, up, down, 0, out_len)
    assert got.dtype == F
    err, bound = np.abs(got.astype(np.float64) - want), _bound(x, h, up, down, 0, out_len)
    print(f"up={up} down={down} nx={nx} nh={nh}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all(), (int(np.argmax(err - bound)), float(np.max(err - bound)))


@pytest.mark.parametrize("up,down,nx,nh", [(3, 2, 50, 31), (160, 441, 900, 8821), (2, 1, 33, 41), (1, 3, 100, 61), (7, 5, 64, 9), (5, 7, 3, 201)])
def test_oracle_against_scipy_resample_poly_float64(up, down, nx, nh):
    """resample_poly's alignment: t0 = (nh - 1) / 2 and ceil(nx up / down) outputs, the taps passed as `window` (scipy multiplies them
    by up), odd nh."""
    from scipy import signal

    rng = np.random.default_rng(27100 + up + nh)
    x = rng.uniform(-1, 1, nx).astype(F)
    w = (np.round(rng.uniform(-1, 1, nh) * 4096) / 4096).astype(F)  # 13 bits: w * up is exact in f32 and in scipy's float64
    h = w * F(up)
    assert (h.astype(np.float64) == w.astype(np.float64) * up).all()
    want = signal.resample_poly(x.astype(np.float64), up, down, window=w.astype(np.float64))
    out_len = -(-nx * up // down)
    assert want.shape == (out_len,)
    t0 = (nh - 1) // 2
    have = min(out_len, max(-(-((nx - 1) * up + nh - t0) // down), 0))
    got = np.zeros(out_len, F)
    got[:have] = ro.resample_ref(x, h, up, down, t0, have)
    bound = np.zeros(out_len)
    bound[:have] = _bound(x, h, up, down, t0, have)
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= bound).all(), (int(np.argmax(err - bound)), float(np.max(err - bound)))


@pytest.mark.parametrize("up,down", [(1, 2), (3, 2), (160, 441), (1, 3), (147, 160), (2, 1)])
def test_taps_against_scipy_firwin(hiplib, up, down):
    from scipy import signal

    from kofft_amd import resample

    mx = max(up, down)
    want64 = signal.firwin(2 * 10 * mx + 1, 1.0 / mx, window=("kaiser", 5.0)) * up
    want = want64.astype(F)
    nh = C.c_size_t()
    assert hiplib.kofft_hip_resample_taps_f32(up, down, 10, 5.0, None, C.byref(nh)) == OK and nh.value == 20 * mx + 1
    got = resample.design_taps(up, down)
    assert got.dtype == F and got.shape == want.shape
    ulp = np.spacing(np.abs(want))
    diff = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ok = (diff <= ulp) | (diff <= 1e-12 * np.max(np.abs(want)))
    print(f"{up}/{down}: {int((got != want).sum())} of {want.size} taps differ from scipy's, worst {diff.max():.3e}")
    assert ok.all(), (int(np.argmax(~ok)), got[~ok][:4], want[~ok][:4])
    assert abs(float(got.astype(np.float64).sum()) - up) <= 1e-5 * up


def test_taps_errors(hiplib):
    nh = C.c_size_t(7)
    buf = np.zeros(64, F)
    f = hiplib.kofft_hip_resample_taps_f32
    assert f(1, 2, 10, 5.0, None, None) == NULL
    for args in [(0, 2, 10, 5.0), (1, 0, 10, 5.0), (1, 2, 0, 5.0), (1, 2, 10, -1.0), (1, 2, 10, float("nan"))]:
        assert f(*args, VP(buf.ctypes.data), C.byref(nh)) == INVALID, args
    assert nh.value == 7 and not buf.any()  # nothing written on an error
    assert f(1 << 62, 1, 10, 5.0, None, C.byref(nh)) == UNSUPPORTED
    assert f(1, 3, 1, 0.0, VP(buf.ctypes.data), C.byref(nh)) == OK and nh.value == 7  # beta 0: a rectangular window
    assert abs(float(buf[:7].astype(np.float64).sum()) - 1.0) < 1e-6


def test_pins_by_hand():
    got = ro.resample_ref(np.array([1, 2, 3], F), np.array([1, 1], F), 2, 1, 0, 6)
    assert got.tobytes() == np.array([1, 1, 2, 2, 3, 3], F).tobytes()
    # up > nh: phases 2 and 3 have no taps, their outputs are +0 (the sign bit too), even with negative data
    got = ro.resample_ref(np.array([-1, -2], F), np.array([1, 1], F), 4, 1, 0, 6)
    assert got.tobytes() == np.array([-1, -1, 0, 0, -2, -2], F).tobytes() and not np.signbit(got[2:4]).any()
    # -0 inputs: +0 + (-0 * h) is +0
    got = ro.resample_ref(np.full(5, -0.0, F), np.array([1, 2, 3], F), 3, 2, 0, ro.full_len(5, 3, 3, 2))
    assert got.tobytes() == np.zeros(got.shape, F).tobytes()
    # skipped, not multiplied by zero: a NaN tap reaches only the outputs that pair it with a sample
    h = np.array([1, np.nan, 1], F)
    got = ro.resample_ref(np.array([1, 1], F), h, 1, 1, 0, 4)
    assert np.isnan(got).tolist() == [False, True, True, False]


def _call(hiplib, name, ctx, x, rows, nx, h, nh, up, down, t0, out, out_len):
    return getattr(hiplib, name)(ctx, x, rows, nx, h, nh, up, down, t0, out, out_len)


@pytest.mark.parametrize("name", ["kofft_hip_resample_f32", "kofft_hip_dev_resample_f32"])
def test_argument_checks_in_the_headers_order_with_a_null_context(hiplib, name):
    """(ctx, x, rows, nx, h, nh, up, down, t0, out, out_len): each line violates one check and every later one it can."""
    buf = np.zeros(64, F)
    p, null, big = VP(buf.ctypes.data), VP(None), (1 << 64) - 1
    call = lambda *a: _call(hiplib, name, null, *a)  # noqa: E731
    assert call(null, 0, 0, null, 0, 0, 0, big, null, 5) == OK            # 1: no rows, whatever else
    assert call(null, 5, 0, null, 0, 0, 0, big, null, 0) == OK            # 1: no outputs
    assert call(null, 2, 0, null, 3, 0, 0, big, null, 5) == EMPTY         # 2: nx == 0 before up == 0
    assert call(null, 2, 4, null, 0, 0, 0, big, null, 5) == EMPTY         # 2: nh == 0
    assert call(null, 2, 1 << 63, null, 3, 0, 4, big, null, 5) == INVALID  # 3: up == 0 before the overflow
    assert call(null, 2, 4, null, 3, 4, 0, big, null, 5) == INVALID       # 3: down == 0
    assert call(null, 2, 1 << 63, null, 3, 4, 1, 0, null, 5) == UNSUPPORTED   # 4: full_up
    assert call(null, 2, 4, null, 3, 1, 1, big, null, 2) == UNSUPPORTED   # 4: t0 + (out_len - 1) down
    assert call(null, 2, 4, null, 3, 1, 1 << 62, 0, null, 5) == UNSUPPORTED   # 4: (out_len - 1) down
    assert call(null, 1 << 62, 4, null, 3, 1, 1, 100, null, 1) == UNSUPPORTED  # 4: a byte count, before the window check
    assert call(null, 2, 4, null, 3, 1, 1, 6, null, 1) == MISMATCH        # 5: full_up = 6: t0 = 6 is past it
    assert call(null, 2, 4, null, 3, 2, 3, 0, null, 4) == MISMATCH        # 5: full_up = 9: outputs at 0, 3, 6, 9
    assert call(null, 2, 4, null, 3, 2, 3, 0, null, 3) == NULL            # 6: the same with 3 outputs is a valid request
    assert call(p, 2, 4, p, 3, 1, 1, 5, p, 1) == NULL                     # 6: the last permitted output, null context
    assert call(p, 2, 4, p, 3, 7, 5, 0, p, 1) == NULL


def test_route_query(hiplib):
    r = C.c_int(7)
    f = hiplib.kofft_hip_resample_route
    assert f(5, 1, 1, None) == NULL
    assert f(0, 1, 1, C.byref(r)) == EMPTY and f(5, 0, 1, C.byref(r)) == INVALID and f(5, 1, 0, C.byref(r)) == INVALID and r.value == 7
    from kofft_amd import resample

    for up, down in [(3, 2), (1, 3), (160, 441)]:
        routes = [resample.route(nh, up, down) for nh in list(range(1, 2000)) + list(range(2000, 200000, 61))]
        assert set(routes) == {0, 1}, (up, down)
        first_plain = routes.index(0)
        assert first_plain > 0 and not any(routes[first_plain:]), f"{up}/{down}: the route is not tiled up to some nh and plain beyond"
    # shapes no LDS holds
    assert resample.route(5, 1, 441) == 0 and resample.route(5, 1 << 40, 1) == 0 and resample.route(1 << 40, 1, 1) == 0
    # the measured rule: the tiled kernel wherever its tables fit
    assert resample.route(61, 1, 3) == 1 and resample.route(8821, 160, 441) == 1 and resample.route(61, 3, 1) == 1
    assert resample.route(41, 2, 1) == 1 and resample.route(64, 1, 1) == 1


def test_python_errors_before_any_device():
    import kofft_amd
    from kofft_amd import resample

    before = resample._default
    E = kofft_amd.FftError
    x = np.ones((2, 10), F)
    h = np.ones(5, F)
    for fn, args, code in [(resample.upfirdn, (h, x, 0, 1), INVALID), (resample.upfirdn, (h, x, 1, 0), INVALID),
                           (resample.upfirdn, (np.ones(0, F), x), EMPTY), (resample.upfirdn, (h, np.ones((2, 0), F)), EMPTY),
                           (resample.resample_poly, (x, 0, 1), INVALID), (resample.resample_poly, (x, 3, 0), INVALID),
                           (resample.resample_poly, (np.ones((2, 0), F), 3, 2), EMPTY), (resample.design_taps, (0, 1), INVALID),
                           (resample.design_taps, (1, 2, 0), INVALID), (resample.design_taps, (1, 2, 10, -1.0), INVALID)]:
        with pytest.raises(E) as e:
            fn(*args)
        assert e.value.code == code, (fn.__name__, args)
    with pytest.raises(E) as e:
        resample.resample_poly(x, 3, 2, taps=np.ones(0, F))
    assert e.value.code == EMPTY
    for fn, args in [(resample.upfirdn, (h, x, -1, 1)), (resample.resample_poly, (x, 1, -2)), (resample.design_taps, (-1, 2))]:
        with pytest.raises(ValueError):
            fn(*args)
    for fn, args in [(resample.upfirdn, (h, np.ones((2, 3, 4), F))), (resample.upfirdn, (np.ones((2, 5), F), x)),
                     (resample.resample_poly, (np.ones((2, 3, 4), F), 3, 2))]:
        with pytest.raises(TypeError):
            fn(*args)
    # 1 / 1 after the gcd: a float32 copy, no device
    src = np.arange(6, dtype=np.float64).reshape(2, 3)
    got = resample.resample_poly(src, 4, 4)
    assert got.dtype == F and got.shape == (2, 3) and (got == src).all() and not np.shares_memory(got, src)
    assert resample.design_taps(3, 2).shape == (61,) and resample.design_taps(4, 6, zeros=2).shape == (25,)
    assert resample._default is before, "a context was created before the errors"


def test_the_plan_arithmetic_under_asan_ubsan(tmp_path):
    """resample_plan.h against an enumeration of every term of every output of every tile, in a stand-alone program under
    AddressSanitizer + UndefinedBehaviorSanitizer."""
    exe = tmp_path / "sanitize_resample_plan"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", *flags, str(ROOT / "tests" / "cpp" / "sanitize_resample_plan.cpp"), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 problems" in res.stdout
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
