"""Welch power spectra and cross spectra of rows without a GPU: the six symbols with their declared argument order,
every argument check of the C ABI in the header's order through a null context (each case is reachable only if the earlier checks
passed: a check that came later would give NULL, the last one before the overlaps), the psd module's errors before any device is
touched, kofft_hip_welch_scale_f32 against a Python loop, the test oracle against scipy in float64, the condition that makes the GPU
grid tell the grouped summation order from a flat one, and the composed route's chunk cutting (kofft_amd/csrc/welch_cut.h) in a
stand-alone program under sanitizers."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import welch_oracle as wo

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
SZ, VP = C.c_size_t, C.c_void_p
# ctx, signal (x, y), rows, len, row_stride, window, win_len, hop, frames, scale, flags, out
WELCH = [VP, VP, SZ, SZ, SZ, VP, SZ, SZ, SZ, C.c_float, C.c_int, VP]
CSD = [VP, VP, VP, SZ, SZ, SZ, VP, SZ, SZ, SZ, C.c_float, C.c_int, VP]
SYMBOLS = {"kofft_hip_welch_f32": WELCH, "kofft_hip_dev_welch_f32": WELCH, "kofft_hip_csd_f32": CSD, "kofft_hip_dev_csd_f32": CSD}
OK, EMPTY, MISMATCH, HOP, INVALID, UNSUPPORTED, NULL = 0, 1, 3, 5, 6, -2, -3


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_symbol_and_declared_argument_order(hiplib, name):
    fn = getattr(hiplib, name)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == SYMBOLS[name]
    assert hiplib.kofft_hip_set_welch_fused.argtypes == [VP, C.c_int]
    assert hiplib.kofft_hip_set_welch_fused(None, 0) == NULL
    assert hiplib.kofft_hip_welch_scale_f32.argtypes == [VP, SZ, C.c_double, SZ, C.c_int, C.POINTER(C.c_float)]


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_checks_in_the_headers_order_with_a_null_context(hiplib, name):
    fn, csd = getattr(hiplib, name), "csd" in name
    buf = np.zeros(256, F)
    p = VP(buf.ctypes.data)

    def call(x=p, y=p, rows=2, length=10, stride=10, win=p, win_len=8, hop=4, frames=3, flags=0, out=p):
        sigs = [x, y] if csd else [x]
        return fn(None, *sigs, rows, length, stride, win, win_len, hop, frames, 1.0, flags, out)

    # the STFT rows' checks, without the frame count
    assert call(hop=0) == HOP
    assert call(hop=0, frames=0, win_len=0, flags=2, out=None) == HOP          # the hop comes first
    assert call(rows=0) == OK and call(rows=0, win_len=0, flags=2, out=None) == OK
    assert call(frames=0) == OK and call(frames=0, win_len=0, flags=2, x=None, out=None) == OK  # nothing to do, nothing touched
    assert call(frames=1) == NULL and call(frames=2) == NULL                   # no lower bound: fewer frames than ceil(len / hop)
    assert call(win_len=0) == EMPTY and call(win_len=0, flags=2, out=None) == EMPTY
    assert call(win_len=(1 << 26) + 1) == UNSUPPORTED and call(win_len=(1 << 25) + 1) == UNSUPPORTED
    assert call(win_len=(1 << 26) + 1, stride=9) == UNSUPPORTED
    assert call(stride=9) == INVALID and call(stride=9, flags=2, out=None) == INVALID
    assert call(rows=1, stride=0) == NULL                                      # one row: the stride is not looked at
    assert call(frames=1 << 62) == UNSUPPORTED and call(frames=1 << 62, flags=2) == UNSUPPORTED  # sizes that overflow
    # then the flags
    assert call(flags=2) == INVALID and call(flags=3) == INVALID and call(flags=-2) == INVALID
    assert call(flags=2, x=None, out=None) == INVALID                          # before the pointers
    # then the pointers: everything passed, only the context is missing
    assert call(x=None) == NULL and call(out=None) == NULL and call() == NULL and call(flags=1) == NULL
    if csd:
        assert call(y=None) == NULL
    assert call(win=None) == NULL                                              # a null window is hann(win_len), not an error
    assert call(x=None, y=None, length=0, stride=0) == NULL                    # no samples: the signals may be null
    assert call(win_len=1) == NULL and call(win_len=5) == NULL and call(win_len=400) == NULL


def test_scale_against_an_ascending_double_loop(hiplib):
    """1 / (fs * sum w^2 * frames) and 1 / ((sum w)^2 * frames): ascending sums in double over the f32 window, rounded to f32 once."""
    from kofft_amd import psd, window

    def want(w, fs, frames, scaling):
        s = 0.0
        for v in w:
            v = float(v)
            s = s + (v * v if scaling == 0 else v)
        return F(1.0 / (fs * s * frames)) if scaling == 0 else F(1.0 / ((s * s) * frames))

    for n in (8, 400, 1024):
        for name, w in (("hann", window.hann(n)), ("hamming", window.hamming(n))):
            w = np.ascontiguousarray(w, F)
            for scaling, word in ((0, "density"), (1, "spectrum")):
                for fs, frames in ((1.0, 1), (16000.0, 37), (44100.0, 112497)):
                    out = C.c_float()
                    assert hiplib.kofft_hip_welch_scale_f32(VP(w.ctypes.data), n, fs, frames, scaling, C.byref(out)) == OK
                    assert F(out.value).tobytes() == want(w, fs, frames, scaling).tobytes(), (name, n, scaling, fs, frames)
                    assert F(psd.scale(w, n, fs, frames, word)).tobytes() == F(out.value).tobytes()
                    if name == "hann":  # a null window is window::hann(win_len)
                        assert hiplib.kofft_hip_welch_scale_f32(None, n, fs, frames, scaling, C.byref(out)) == OK
                        assert F(out.value).tobytes() == want(w, fs, frames, scaling).tobytes()
    out = C.c_float(7.0)
    w = np.ones(8, F)
    p = VP(w.ctypes.data)
    assert hiplib.kofft_hip_welch_scale_f32(p, 8, 1.0, 1, 0, None) == NULL
    assert hiplib.kofft_hip_welch_scale_f32(p, 0, 1.0, 1, 0, C.byref(out)) == EMPTY
    for fs, frames, scaling in ((0.0, 1, 0), (-1.0, 1, 0), (float("nan"), 1, 1), (1.0, 0, 0), (1.0, 1, 2), (1.0, 1, -1)):
        assert hiplib.kofft_hip_welch_scale_f32(p, 8, fs, frames, scaling, C.byref(out)) == INVALID
    z = np.zeros(8, F)
    assert hiplib.kofft_hip_welch_scale_f32(VP(z.ctypes.data), 8, 1.0, 1, 0, C.byref(out)) == INVALID  # a zero sum
    pm = np.ascontiguousarray([1, -1] * 4, F)
    assert hiplib.kofft_hip_welch_scale_f32(VP(pm.ctypes.data), 8, 1.0, 1, 1, C.byref(out)) == INVALID
    assert out.value == 7.0  # nothing written on an error


def test_python_errors_before_any_device():
    import kofft_amd
    from kofft_amd import psd

    before = psd._default
    x = np.ones((2, 100), F)
    E = kofft_amd.FftError
    for args, kw, code in [((x, 64), dict(hop=0), HOP), ((x, 0), {}, EMPTY), ((x, 128), {}, MISMATCH), ((x, 64), dict(fs=0.0), INVALID),
                           ((x, 64), dict(fs=float("nan")), INVALID)]:
        with pytest.raises(E) as e:
            psd.welch(*args, **kw)
        assert e.value.code == code
        with pytest.raises(E) as e:
            psd.csd(args[0], *args, **kw)
        assert e.value.code == code
    with pytest.raises(E) as e:
        psd.welch(x, 64, window=np.zeros(64, F))  # a zero window has no scale
    assert e.value.code == INVALID
    with pytest.raises(ValueError):
        psd.welch(x, 64, scaling="power")
    with pytest.raises(ValueError):
        psd.welch(x, -4)
    with pytest.raises(TypeError):
        psd.welch(np.ones((2, 3, 100), F), 64)
    with pytest.raises(TypeError):
        psd.welch(x, 64, window=np.ones(63, F))
    with pytest.raises(TypeError):
        psd.csd(x, np.ones((3, 100), F), 64)
    assert psd.segments(100, 64, 32) == 2 and psd.segments(63, 64, 32) == 0 and psd.segments(64, 64, 1000) == 1
    assert psd.segments(4096, 256, 128) == 31
    with pytest.raises(E):
        psd.segments(100, 64, 0)
    assert psd._default is before, "a context was created before the errors"


# The oracle in f32 against scipy in float64, detrend=False, the periodic Hann window, hop = win_len / 2, density scaling, one-sided and
# doubled: the largest error relative to the spectrum's peak.  It is the f32 twiddle drift of the reference's table recurrence (SURVEY 8
# a2) and varies with the data; measured on these two inputs (seeds below) and allowed four times that.
#   (len, win_len):  welch measured,  csd measured
SCIPY_MEASURED = {(4096, 256): (9.893e-7, 1.007e-6), (20000, 1024): (3.706e-5, 4.129e-5)}


@pytest.mark.parametrize("length,win_len", sorted(SCIPY_MEASURED))
def test_oracle_against_scipy_float64(oracle, hiplib, length, win_len):
    from scipy import signal
    hop = win_len // 2
    rng = np.random.default_rng(26500 + win_len)
    x = rng.standard_normal((1, length)).astype(F)
    y = (0.5 * x + rng.standard_normal((1, length))).astype(F)
    win = signal.get_window("hann", win_len).astype(F)  # periodic
    frames = (length - win_len) // hop + 1
    scale = C.c_float()
    assert hiplib.kofft_hip_welch_scale_f32(VP(win.ctypes.data), win_len, 1.0, frames, 0, C.byref(scale)) == OK
    kw = dict(fs=1.0, window=win.astype(np.float64), nperseg=win_len, noverlap=win_len - hop, detrend=False, scaling="density")
    _, p64 = signal.welch(x[0].astype(np.float64), **kw)
    _, c64 = signal.csd(x[0].astype(np.float64), y[0].astype(np.float64), **kw)
    p32 = wo.welch_ref(x, win, hop, frames, scale.value, True)[0]
    c32 = wo.welch_ref(x, win, hop, frames, scale.value, True, y=y)[0]
    err_p = float(np.max(np.abs(p32 - p64)) / np.max(p64))
    err_c = float(np.max(np.abs(c32 - c64)) / np.max(np.abs(c64)))
    print(f"len={length} win_len={win_len}: welch {err_p:.3e} csd {err_c:.3e} of the peak")
    bound_p, bound_c = (4 * m for m in SCIPY_MEASURED[(length, win_len)])
    assert err_p <= bound_p and err_c <= bound_c, (err_p, err_c)


@pytest.mark.parametrize("win_len", wo.GRID_WINS)
def test_the_grid_inputs_tell_the_grouped_order_from_a_flat_one(oracle, win_len):
    """For the 65-frame inputs of tests/test_gpu_welch.py's grid, every row: the contract's two-level sum and one flat ascending sum
    differ in at least one bit of at least one bin, for the power spectrum and (where the GPU grid runs it) the cross spectrum -- a
    kernel that sums in the wrong order cannot pass there.  At 33 frames the two orders are the same sum by construction (the second
    group is one frame, and +0 + p is p), so no seed can tell them apart: that is asserted too, as a property of the contract."""
    win = np.ascontiguousarray(np.hanning(win_len + 1)[:-1], F)
    for frames in (33, 65):
        for rows in wo.GRID_ROWS:
            for hop in wo.grid_hops(win_len):
                x = wo.grid_input(win_len, hop, frames, rows)
                y = wo.grid_input(win_len, hop, frames, rows, 1)
                for r in range(rows):
                    X = wo.frames_of(x[r], win, hop, frames)
                    t = wo._terms(X, None)
                    if frames == 33:
                        assert wo.grouped_sum(t).tobytes() == wo.flat_sum(t).tobytes(), (win_len, frames, rows, hop, r)
                        continue
                    assert wo.grouped_sum(t).tobytes() != wo.flat_sum(t).tobytes(), (win_len, frames, rows, hop, r)
                    if win_len in (64, 1024):
                        c = wo._terms(X, wo.frames_of(y[r], win, hop, frames))
                        g, f = wo.grouped_sum(c), wo.flat_sum(c)
                        assert g.real.tobytes() != f.real.tobytes() and g.imag.tobytes() != f.imag.tobytes(), (win_len, frames, rows, hop, r)


def test_the_chunk_cutting_under_asan_ubsan(tmp_path):
    """welch_cut.h against an enumeration of every frame: every frame in exactly one piece, every piece made of whole groups, in a
    stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer."""
    exe = tmp_path / "sanitize_welch_cut"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", *flags, str(ROOT / "tests" / "cpp" / "sanitize_welch_cut.cpp"), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert res.returncode == 0, res.stdout + res.stderr
    assert "0 problems" in res.stdout
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
