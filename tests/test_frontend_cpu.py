"""The audio front end (rows of samples -> mel energies / MFCCs in one call) without a GPU: the four symbols with their declared
argument order, every argument check of the C ABI in the header's order through a null context (each case is reachable only if the
earlier checks passed: a check that came later would give NULL, the last one), the Python module's errors before any device is
touched, and the fused kernel's per-filter walk (kofft_amd/csrc/frontend_walk.h) in a stand-alone program under sanitizers."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
SZ, VP = C.c_size_t, C.c_void_p
# ctx, signal, rows, len, row_stride, window, win_len, hop, frames, bins, num_mel, [num_coeffs,] out
MEL = [VP, VP, SZ, SZ, SZ, VP, SZ, SZ, SZ, VP, SZ, VP]
MFCC = [VP, VP, SZ, SZ, SZ, VP, SZ, SZ, SZ, VP, SZ, SZ, VP]
SYMBOLS = {"kofft_hip_stft_mel_f32": MEL, "kofft_hip_dev_stft_mel_f32": MEL, "kofft_hip_stft_mfcc_f32": MFCC,
           "kofft_hip_dev_stft_mfcc_f32": MFCC}
OK, EMPTY, MISMATCH, HOP, INVALID, UNSUPPORTED, NULL = 0, 1, 3, 5, 6, -2, -3


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_symbol_and_declared_argument_order(hiplib, name):
    fn = getattr(hiplib, name)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == SYMBOLS[name]
    assert hiplib.kofft_hip_set_frontend_fused.argtypes == [VP, C.c_int]
    assert hiplib.kofft_hip_set_frontend_fused(None, 0) == NULL


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_checks_in_the_headers_order_with_a_null_context(hiplib, name):
    fn, mfcc = getattr(hiplib, name), "mfcc" in name
    buf = np.zeros(256, F)
    p = VP(buf.ctypes.data)
    good = np.ascontiguousarray([0, 1, 2, 4], np.uint64)
    bad = np.ascontiguousarray([0, 2, 1, 4], np.uint64)
    many = np.ascontiguousarray(np.arange(4099), np.uint64)
    g, b, lb = (VP(a.ctypes.data) for a in (good, bad, many))

    def call(sig=p, rows=2, length=10, stride=10, win=p, win_len=8, hop=4, frames=3, bins=g, num_mel=2, nc=2, out=p):
        args = [None, sig, rows, length, stride, win, win_len, hop, frames, bins, num_mel]
        return fn(*args, nc, out) if mfcc else fn(*args, out)

    # the STFT rows' checks
    assert call(hop=0) == HOP
    assert call(hop=0, frames=0, win_len=0, bins=None) == HOP                  # the hop comes first
    assert call(frames=2) == MISMATCH and call(frames=2, win_len=0) == MISMATCH  # both forms: frames < ceil(len / hop)
    assert call(rows=0) == OK and call(rows=0, win_len=0, bins=None, out=None) == OK
    assert call(length=0, stride=0, frames=0, bins=None, nc=9) == OK           # no frames: nothing to do, nothing touched
    assert call(win_len=0) == EMPTY and call(win_len=0, nc=9, bins=None) == EMPTY
    assert call(win_len=(1 << 26) + 1) == UNSUPPORTED and call(win_len=(1 << 25) + 1) == UNSUPPORTED
    assert call(win_len=(1 << 26) + 1, stride=9) == UNSUPPORTED
    assert call(stride=9) == INVALID and call(stride=9, bins=None) == INVALID
    assert call(rows=1, stride=0) == NULL                                      # one row: the stride is not looked at
    # then the mel ones
    if mfcc:
        assert call(nc=3) == INVALID and call(nc=3, bins=None) == INVALID     # num_coeffs > num_mel before null bins
    assert call(bins=None) == NULL
    assert call(bins=None, sig=None, out=None) == NULL
    assert call(bins=b) == INVALID and call(bins=b, win_len=1 << 26) == INVALID  # order before the bounds
    assert call(bins=lb, num_mel=4097, nc=13) == UNSUPPORTED
    assert call(win_len=1 << 26) == UNSUPPORTED                                # win_len / 2 > 2^24: the mel stage's bound
    assert call(bins=lb, num_mel=4097, nc=13, sig=None, out=None) == UNSUPPORTED  # the bounds before the pointers
    assert call(sig=None) == NULL and call(out=None) == NULL and call() == NULL  # everything passed: only the context is missing
    assert call(win=None) == NULL                                              # a null window is hann(win_len), not an error
    assert call(num_mel=0, nc=0) == NULL                                       # valid calls: the null context is reported
    assert call(nc=0) == NULL
    assert call(win_len=1) == NULL


def test_python_errors_before_any_device():
    import kofft_amd
    from kofft_amd import api, mfcc

    before = api._direct_default
    x = np.ones((2, 100), F)
    with pytest.raises(kofft_amd.FftError) as e:
        mfcc.mfcc_from_audio(x, 16000.0, 64, 0, 8, 4)
    assert e.value.code == HOP
    with pytest.raises(kofft_amd.FftError) as e:
        mfcc.mel_from_audio(x, 16000.0, 64, 16, 8, frames=6)  # ceil(100 / 16) = 7
    assert e.value.code == MISMATCH
    with pytest.raises(kofft_amd.FftError) as e:
        mfcc.mel_from_audio(x, 16000.0, 0, 16, 8)
    assert e.value.code == EMPTY
    with pytest.raises(kofft_amd.DeviceError):
        mfcc.mel_from_audio(x, 16000.0, (1 << 26) + 1, 16, 8, bins=list(range(10)))
    with pytest.raises(kofft_amd.FftError) as e:
        mfcc.mfcc_from_audio(x, 16000.0, 64, 16, 8, 20)
    assert e.value.code == INVALID
    with pytest.raises(kofft_amd.FftError) as e:
        mfcc.mel_from_audio(x, 16000.0, 64, 16, 2, bins=[0, 5, 3, 9])
    assert e.value.code == INVALID
    with pytest.raises(kofft_amd.FftError) as e:
        mfcc.mel_from_audio(x, 16000.0, 64, 16, 2, bins=[0, 3, 9])  # not num_filters + 2 edges
    assert e.value.code == MISMATCH
    with pytest.raises(kofft_amd.DeviceError):
        mfcc.mel_from_audio(x, 16000.0, 64, 16, 4097)
    with pytest.raises(TypeError):
        mfcc.mel_from_audio(np.ones((2, 3, 4), F), 16000.0, 64, 16, 8)
    with pytest.raises(TypeError):
        mfcc.mel_from_audio(x, 16000.0, 64, 16, 8, window=np.ones(63, F))
    with pytest.raises(TypeError):
        mfcc.mel_from_audio(x, 16000.0, 64, 16, 2, bins=[0.0, 1.0, 2.0, 3.0])
    with pytest.raises(ValueError):
        mfcc.mfcc_from_audio(x, 16000.0, 64, 16, 8, -1)
    assert api._direct_default is before, "a context was created before the errors"


def test_the_filter_walk_under_asan_ubsan(tmp_path):
    """frontend_walk.h over mel_plan_build's plans against the reference's two loops, bit for bit, in a stand-alone program under
    AddressSanitizer + UndefinedBehaviorSanitizer."""
    exe = tmp_path / "sanitize_frontend_walk"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-ffp-contract=off"]
    subprocess.run(["g++", "-std=c++17", *flags, str(ROOT / "tests" / "cpp" / "sanitize_frontend_walk.cpp"),
                    str(ROOT / "kofft_amd" / "csrc" / "tables.cpp"), "-lm", "-pthread", "-o", str(exe)], check=True, capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert res.returncode == 0, res.stdout + res.stderr
    assert "0 problems" in res.stdout
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
