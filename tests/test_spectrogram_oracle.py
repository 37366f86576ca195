"""visual::spectrogram's colour helpers on the host side (no GPU): the reference's own four tests restated as numbers on the oracle
(tests/spectrogram_oracle.py), the crate's log10f at the powers of ten and against float64, the library's host helpers
kofft_hip_log_bin_map / kofft_hip_map_color_u8 against the oracle, the argument checks of the C ABI in their order through a null
context, the Python module's errors before any device, the range builder in a stand-alone program under sanitizers, and the record of
how far a glibc-shaped log10 moves the pixels."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import spectrogram_oracle as so

ROOT = Path(__file__).resolve().parent.parent
F = np.float32

_libm = C.CDLL("libm.so.6")
_libm.powf.restype = C.c_float
_libm.powf.argtypes = [C.c_float, C.c_float]


def _pow10(e) -> np.float32:
    return F(_libm.powf(F(10.0), F(e)))


def test_the_references_own_tests_on_the_oracle():
    """spectrogram.rs:240-279 with max_mag 1 and floor -120."""
    floor, mx = F(-120.0), F(1.0)
    assert abs(float(so.magnitude_to_db([mx], mx, floor)[0])) < 1e-6
    mag_floor = mx * _pow10(floor / F(20.0))
    assert abs(float(so.magnitude_to_db([mag_floor], mx, floor)[0]) - float(floor)) < 1e-3
    mag_mid = mx * _pow10((floor / F(2.0)) / F(20.0))
    assert abs(float(so.magnitude_to_db([mag_mid], mx, floor)[0]) - float(floor) / 2) < 1e-3
    fire = so.map_color_u8(so.color_t(np.array([mag_floor, mx], F), mx, 0, floor), so.FIRE)
    assert fire.tolist() == [[0, 0, 0], [255, 255, 255]]
    r, g, b = (int(v) for v in so.map_color_u16([0.375], so.RAINBOW)[0])
    assert r == 0 and b == 65535 and 0 < g < 65535
    frame = np.arange(1, 9, dtype=F).reshape(1, 8)
    scaled = so.log_scale_bins(frame, so.log_bin_map(8))
    assert abs(float(scaled[0, 6]) - 6.5) < 1e-6
    assert scaled[0, 6] == F(6.5)


def test_log10f_of_the_powers_of_ten_is_exact():
    for k in range(8):
        x = F(1.0) / F(10 ** k)  # 10f32.powi(-k)
        assert so.libm_log10f([x])[0] == F(-k), k
    assert so.libm_log10f([F(10 ** 7)])[0] == F(7.0)


def test_log10f_specials_and_accuracy():
    with np.errstate(all="ignore"):
        got = so.libm_log10f(np.array([0.0, -0.0, -1.0, np.inf, np.nan, 1.0, 1e-45, 1e-39], F))
    assert got[0] == -np.inf and got[1] == -np.inf and np.isnan(got[2]) and got[3] == np.inf and np.isnan(got[4])
    assert got[5] == 0.0 and not np.signbit(got[5])
    assert abs(float(got[6]) - np.log10(float(F(1e-45)))) < 1e-5 and abs(float(got[7]) - np.log10(float(F(1e-39)))) < 1e-5
    rng = np.random.default_rng(522)
    x = np.exp(rng.uniform(-30.0, 3.0, 400_000)).astype(F)
    exact = np.log10(x.astype(np.float64))
    got = so.libm_log10f(x).astype(np.float64)
    ulp = np.spacing(np.abs(exact).astype(F)).astype(np.float64)
    worst = float(np.max(np.abs(got - exact) / ulp))
    print(f"log10f: worst error {worst:.3f} ulp on {x.size} samples over e^-30 .. e^3")
    assert worst < 1.0  # the libm crate's log10f is a < 1 ulp function (0.83 measured on 4e6 samples)


@pytest.mark.parametrize("bins", [1, 2, 8, 16, 512, 8192])
def test_log_bin_map_is_the_oracles(hiplib, bins):
    out = np.full(bins, 0xFFFFFFFF, np.uint32)
    assert hiplib.kofft_hip_log_bin_map(bins, C.c_void_p(out.ctypes.data)) == 0
    want = so.log_bin_map(bins)
    assert out.tolist() == want.tolist()
    assert np.all(out[1:] >= out[:-1]) and int(out.max()) < bins
    if bins == 16:
        assert int(out[15]) == 14, "at 16 bins the top pixel is 14, not 15"
    if bins == 8:
        assert out.tolist()[5:] == [6, 6, 7]  # what the reference's own test relies on: bins 5 and 6 (values 6 and 7) share pixel 6


def test_log_bin_map_errors(hiplib):
    buf = np.zeros(4, np.uint32)
    p = C.c_void_p(buf.ctypes.data)
    assert hiplib.kofft_hip_log_bin_map(0, p) == 1
    assert hiplib.kofft_hip_log_bin_map((1 << 24) + 1, p) == -2
    assert hiplib.kofft_hip_log_bin_map(4, None) == -3


@pytest.mark.parametrize("cmap", so.IMPLEMENTED)
def test_map_color_u8_is_the_oracles(hiplib, cmap):
    t = np.concatenate([np.arange(4097, dtype=F) / F(4096.0), np.array([np.nan, -1.0, 2.0, 0.9, -0.0, np.inf, -np.inf], F)])
    want = so.map_color_u8(t, cmap)
    got = np.zeros((t.size, 3), np.uint8)
    rgb = (C.c_ubyte * 3)()
    for i, v in enumerate(t):
        assert hiplib.kofft_hip_map_color_u8(float(v), cmap, rgb) == 0
        got[i] = rgb[0], rgb[1], rgb[2]
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"cmap {cmap}: {bad.size} of {t.size} differ, first t={t[bad[0]]!r}: {got[bad[0]]} != {want[bad[0]]}"
    assert got[4097].tolist() == [0, 0, 0]  # NaN: every cast gives 0
    if cmap == so.LEGACY:
        assert got[4098].tolist() == [64, 0, 64] and got[4099].tolist() == [255, 255, 224]


def test_map_color_u8_errors(hiplib):
    rgb = (C.c_ubyte * 3)()
    for cmap in (so.VIRIDIS, so.PLASMA, so.INFERNO, 7, -1):
        assert hiplib.kofft_hip_map_color_u8(0.5, cmap, rgb) == 6
    assert hiplib.kofft_hip_map_color_u8(0.5, so.FIRE, None) == -3


def test_argument_checks_in_order_with_a_null_context(hiplib):
    """include/kofft_hip.h: empty input, the enums, the table, the bounds, then null pointers and context -- no context needed; the
    overlap check (device forms) comes after the null context and is tested on the GPU."""
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    good = np.array([0, 1, 1, 3], np.uint32)
    over = np.array([0, 1, 2, 4], np.uint32)
    down = np.array([0, 2, 1, 3], np.uint32)
    g, o, d = (C.c_void_p(a.ctypes.data) for a in (good, over, down))
    for name in ("kofft_hip_magnitude_to_db_f32", "kofft_hip_dev_magnitude_to_db_f32", "kofft_hip_db_scale_f32", "kofft_hip_dev_db_scale_f32"):
        fn = getattr(hiplib, name)
        assert fn(None, None, 0, None, -120.0, None) == 1   # count == 0 before everything
        assert fn(None, p, 4, p, -120.0, p) == -3           # the null context
        assert fn(None, None, 4, None, -120.0, None) == -3
    for name in ("kofft_hip_spectrogram_render_f32", "kofft_hip_dev_spectrogram_render_f32"):
        fn = getattr(hiplib, name)

        def call(frames=2, bins=4, mode=0, cmap=0, depth=8, scale=0, layout=0, table=None, ptr=None):
            return fn(None, ptr, frames, bins, ptr, mode, -120.0, cmap, depth, scale, layout, table, ptr)

        assert call(frames=0, cmap=9) == 1 and call(bins=0, depth=7) == 1       # empty before the enums
        for kw in ({"mode": 2}, {"mode": -1}, {"cmap": 3}, {"cmap": 4}, {"cmap": 5}, {"cmap": 7}, {"cmap": -1}, {"depth": 0}, {"depth": 24},
                   {"scale": 2}, {"layout": 2}, {"layout": -1}):
            assert call(**kw) == 6, kw                                          # the enums
        assert call(scale=1) == 6                                               # a null table
        assert call(scale=1, table=o) == 6 and call(scale=1, table=d) == 6      # an entry >= bins; a decreasing table
        assert call(bins=(1 << 24) + 1) == -2                                   # the bounds before the pointers
        assert call(frames=1 << 40, bins=1 << 20) == -2
        assert call(scale=1, table=g) == -3 and call() == -3 and call(ptr=p) == -3  # then null data, then the null context
    assert hiplib.kofft_hip_set_spectrogram_transpose(None, 0) == -3


def test_python_errors_before_any_device():
    import kofft_amd
    from kofft_amd import api, spectrogram as sp

    before = api._direct_default
    x = np.ones((4, 8), F)
    for cmap in ("viridis", "plasma", "inferno"):
        with pytest.raises(kofft_amd.FftError) as e:
            sp.map_color_u8(0.5, cmap)
        assert e.value.code == 6
    with pytest.raises(ValueError):
        sp.map_color_u8(0.5, "jet")
    with pytest.raises(kofft_amd.FftError) as e:
        sp.render(np.ones((0, 8), F), 1.0)
    assert e.value.code == 1
    with pytest.raises(kofft_amd.FftError):
        sp.render(x, 1.0, depth=12)
    with pytest.raises(kofft_amd.FftError):
        sp.render(x, 1.0, scale="log", pix_of_bin=[0, 1, 2])
    with pytest.raises(TypeError):
        sp.render(np.ones(8, F), 1.0)
    with pytest.raises(ValueError):
        sp.render(x, 1.0, layout="sideways")
    assert sp.log_bin_map(16).tolist() == so.log_bin_map(16).tolist()
    assert sp.map_color_u8(0.375, sp.RAINBOW).tolist() == so.map_color_u8([0.375], so.RAINBOW)[0].tolist()
    assert api._direct_default is before, "a context was created before the errors"


def test_range_builder_under_asan_ubsan(tmp_path):
    """kofft_tables::log_bin_map and spec_ranges_build in a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer."""
    exe = tmp_path / "sanitize_spectrogram_plan"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-ffp-contract=off"]
    subprocess.run(["g++", "-std=c++17", *flags, str(ROOT / "tests" / "cpp" / "sanitize_spectrogram_plan.cpp"),
                    str(ROOT / "kofft_amd" / "csrc" / "tables.cpp"), "-lm", "-pthread", "-o", str(exe)], check=True, capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert res.returncode == 0, res.stdout + res.stderr
    assert "0 problems" in res.stdout and "at most 9" in res.stdout
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr


def test_glibc_shaped_log10_moves_pixels_only_where_the_logs_differ():
    """A record, not a gate: the oracle's pixels against a twin whose log10 is numpy's float32 log10, on one 64 x 512
    frame set.  Asserted: every differing pixel lies where the two log10 values differ."""
    rng = np.random.default_rng(5220)
    mags = (10.0 ** rng.uniform(-7.0, 0.0, (64, 512))).astype(F)
    mx = F(mags.max())
    for mode, level in ((0, -120.0), (1, 80.0)):
        with np.errstate(all="ignore"):
            ratio = (mags / mx).reshape(-1)
            arg = ratio if mode == 0 else so.rust_max(ratio, F(1e-10))
            logs_differ = so.libm_log10f(arg).view(np.uint32) != np.log10(arg).astype(F).view(np.uint32)
        for cmap in so.IMPLEMENTED:
            a = so.render(mags, mx, mode, level, cmap, 8, 0, 0)
            b = so.render(mags, mx, mode, level, cmap, 8, 0, 0, log10=np.log10)
            px_differ = (a != b).any(axis=2).reshape(-1)
            assert not np.any(px_differ & ~logs_differ), "a pixel moved where the two log10 agree"
            print(f"mode {mode} cmap {cmap}: log10 differs at {logs_differ.mean():.4f} of the arguments, pixels at {px_differ.mean():.6f}")
