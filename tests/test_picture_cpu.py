"""Audio -> spectrogram pictures in one call (kofft_hip_stft_picture_f32 and its kofft_hip_dev_ form) without a GPU: the two symbols
with their declared argument order, every argument check of the C ABI in the header's order through a null context (each case is
reachable only if the earlier checks passed: a check that came later would give NULL, the last one), the Python module's errors before
any device is touched, the oracle's running maximum against a literal restatement of compute_frame, and the chunk cutting
(kofft_amd/csrc/frame_cut.h, with the chunk walk and the overlap test of host_layout.h) in a stand-alone program under sanitizers."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import picture_oracle as po

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
SZ, VP, I = C.c_size_t, C.c_void_p, C.c_int
# ctx, signal, rows, len, row_stride, window, win_len, hop, frames, max_mode, max_in, max_out, mode, level, cmap, depth, channels, scale,
# layout, pix_of_bin, out
PICTURE = [VP, VP, SZ, SZ, SZ, VP, SZ, SZ, SZ, I, VP, VP, I, C.c_float, I, I, I, I, I, VP, VP]
SYMBOLS = ["kofft_hip_dev_stft_picture_f32", "kofft_hip_stft_picture_f32"]
OK, EMPTY, MISMATCH, HOP, INVALID, UNSUPPORTED, NULL = 0, 1, 3, 5, 6, -2, -3


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_and_declared_argument_order(hiplib, name):
    fn = getattr(hiplib, name)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == PICTURE
    header = (ROOT / "include" / "kofft_hip.h").read_text()
    assert f"int {name}(kofft_hip_ctx *ctx, const float *" in header
    proto = header[header.index(f"int {name}("):]
    proto = proto[:proto.index(";")]
    import re

    names = [re.sub(r"^d_", "", n) for n in re.findall(r"(\w+)\s*[,)]", re.sub(r"/\*.*?\*/", "", proto))]
    at = names
    order = ["ctx", "signal", "rows", "len", "row_stride", "window", "win_len", "hop", "frames", "max_mode", "max_in", "max_out", "mode", "level",
             "cmap", "depth", "channels", "scale", "layout", "pix_of_bin", "out"]
    assert at == order, "the prototype's argument order"


@pytest.mark.parametrize("name", SYMBOLS)
def test_checks_in_the_headers_order_with_a_null_context(hiplib, name):
    fn, dev = getattr(hiplib, name), "_dev_" in name
    buf = np.zeros(256, F)
    mx = np.full(4, 7.0, F)
    p, pm = VP(buf.ctypes.data), VP(mx.ctypes.data)
    good = np.ascontiguousarray([0, 1, 2, 3], np.uint32)
    high = np.ascontiguousarray([0, 1, 2, 4], np.uint32)
    down = np.ascontiguousarray([0, 2, 1, 3], np.uint32)
    g, h, d = (VP(a.ctypes.data) for a in (good, high, down))

    def call(sig=p, rows=2, length=10, stride=10, win=p, win_len=8, hop=4, frames=3, max_mode=0, max_in=None, max_out=None, mode=0, level=-80.0,
             cmap=0, depth=8, channels=3, scale=0, layout=1, table=None, out=p):
        return fn(None, sig, rows, length, stride, win, win_len, hop, frames, max_mode, max_in, max_out, mode, level, cmap, depth, channels, scale,
                  layout, table, out)

    # 1. the STFT rows' checks
    assert call(hop=0) == HOP
    assert call(hop=0, frames=0, win_len=0, mode=9, max_mode=9) == HOP            # the hop comes first
    assert call(frames=2) == MISMATCH and call(frames=2, win_len=0, cmap=3) == MISMATCH
    assert call(rows=0) == OK and call(rows=0, win_len=0, mode=9, max_mode=9, out=None) == OK
    assert call(length=0, stride=0, frames=0, channels=7) == OK                   # no frames: nothing to do, nothing touched
    assert call(win_len=0) == EMPTY and call(win_len=0, depth=9, max_mode=9) == EMPTY
    assert call(win_len=(1 << 26) + 1) == UNSUPPORTED and call(win_len=(1 << 25) + 1, mode=9) == UNSUPPORTED
    assert call(stride=9) == INVALID and call(stride=9, out=None) == INVALID
    assert call(rows=1, stride=0) == NULL                                         # one row: the stride is not looked at
    # 2. the render's enums and its table
    for bad in (dict(mode=2), dict(mode=-1), dict(cmap=3), dict(cmap=4), dict(cmap=5), dict(cmap=7), dict(cmap=-1), dict(depth=12), dict(scale=2),
                dict(layout=2), dict(layout=-1)):
        assert call(**bad) == INVALID, bad
        assert call(**bad, sig=None, out=None, win_len=1 << 26) == INVALID, bad   # before the bound, the empty case and the pointers
    assert call(scale=1) == INVALID and call(scale=1, table=h) == INVALID and call(scale=1, table=d) == INVALID
    assert call(scale=1, table=g) == NULL                                         # a good table: only the context is missing
    # 3. this call's own
    for bad in (dict(max_mode=3), dict(max_mode=-1), dict(channels=2), dict(channels=5), dict(channels=4, depth=16),
                dict(max_mode=1, scale=1, table=g)):
        assert call(**bad) == INVALID, bad
        assert call(**bad, sig=None, out=None) == INVALID, bad                    # before the pointers
    assert call(max_mode=3, win_len=1) == INVALID                                 # before the empty case
    assert call(win_len=1 << 26) == UNSUPPORTED and call(win_len=1 << 26, out=None) == UNSUPPORTED  # win_len / 2 > 2^24
    # 4. no bins: nothing but max_out is written, and nothing else is looked at
    if dev:
        assert call(win_len=1, sig=None, out=None) == OK                          # max_out null: nothing to write
        assert call(win_len=1, max_out=pm) == NULL                                # something to write: the device form needs the context
        assert call(win_len=1, max_mode=2, max_in=None) == NULL
    else:
        for max_mode, want in ((0, F(0.0)), (1, F(1e-12))):
            mx[:] = 7.0
            assert call(win_len=1, hop=5, frames=2, max_mode=max_mode, max_out=pm, sig=None, out=None) == OK
            assert mx[0].tobytes() == want.tobytes() and mx[1].tobytes() == want.tobytes() and mx[2] == 7.0
        given = np.ascontiguousarray([3.5, np.nan], F)
        assert call(win_len=1, max_mode=2, max_in=VP(given.ctypes.data), max_out=pm) == OK
        assert mx[:2].tobytes() == given.tobytes() and mx[2] == 7.0
        assert call(win_len=1, max_mode=2, max_in=None, max_out=pm) == NULL
        assert call(win_len=1, max_out=None) == OK
    # 5. null pointers: everything passed, only the context (or a pointer) is missing
    assert call(sig=None) == NULL and call(out=None) == NULL and call() == NULL
    assert call(max_mode=2, max_in=None) == NULL and call(max_mode=2, max_in=pm) == NULL
    assert call(win=None) == NULL                                                 # a null window is hann(win_len), not an error
    assert call(channels=4) == NULL and call(depth=16) == NULL and call(max_mode=1, max_out=pm) == NULL
    assert buf.tobytes() == bytes(buf.nbytes), "no call wrote a byte of the picture"


def test_python_errors_before_any_device():
    import kofft_amd
    from kofft_amd import api, spectrogram

    before = api._direct_default
    x = np.ones((2, 100), F)
    cases = [(dict(hop=0), HOP), (dict(frames=6), MISMATCH), (dict(max_mode=1, scale="log"), INVALID), (dict(channels=4, depth=16), INVALID),
             (dict(channels=2), INVALID), (dict(depth=12), INVALID), (dict(scale="log", pix_of_bin=[0, 1, 2]), MISMATCH)]
    for kw, code in cases:
        args = dict(win_len=64, hop=16)
        args.update(kw)
        with pytest.raises(kofft_amd.FftError) as e:
            spectrogram.from_audio(x, args.pop("win_len"), args.pop("hop"), **args)
        assert e.value.code == code, kw
    with pytest.raises(ValueError):
        spectrogram.from_audio(x, 64, 16, max_mode="loudest")
    with pytest.raises(ValueError):
        spectrogram.from_audio(x, 64, 16, cmap="jet")
    with pytest.raises(TypeError):
        spectrogram.from_audio(x, 64, 16, max_mode="given")
    with pytest.raises(TypeError):
        spectrogram.from_audio(np.ones((2, 3, 4), F), 64, 16)
    assert api._direct_default is before, "a context was created before the errors"


def test_running_maximum_against_compute_frame_restated():
    """3 frames of 8 bins with a NaN and an inf: the accumulate form of tests/picture_oracle.py against the scalar loop, bit for bit; the
    row maximum skips the NaN too."""
    rng = np.random.default_rng(7)
    m = np.abs(rng.standard_normal((3, 8))).astype(F) * F(1e-3)
    m[0, :3] = [0.0, 1e-13, 5e-13]          # below the seed: the seed shows
    m[0, 5] = np.nan
    m[1, 2] = 4.0
    m[2, 6] = np.inf
    want, last = po.compute_frame_literal(m)
    got = po.running_max(m)
    assert got.tobytes() == want.tobytes()
    assert got[0, 0] == F(1e-12) and got[0, 2] == F(1e-12) and got[0, 5] == got[0, 4] and not np.isnan(got).any()
    assert np.isinf(got[2, 6:]).all() and np.isfinite(got[2, :6]).all() and np.isinf(last)
    assert po.row_max(m[:2]) == F(4.0) and np.isinf(po.row_max(m)) and po.row_max(np.full((2, 2), np.nan, F)).tobytes() == F(0.0).tobytes()
    px, mx = po.pictures(m[None], max_mode=1, mode=0, level=-80.0, cmap=6, channels=4, layout=0)
    assert px.shape == (1, 3, 8, 4) and (px[..., 3] == 255).all() and np.isinf(mx[0])


def test_the_chunk_cutting_under_asan_ubsan(tmp_path):
    """frame_cut.h against an enumeration of every frame of every chunk that for_chunks hands out, and overlaps / rows_span against
    enumerations of bytes, in a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer."""
    exe = tmp_path / "sanitize_frame_cut"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", *flags, str(ROOT / "tests" / "cpp" / "sanitize_frame_cut.cpp"), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 problems" in res.stdout
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
