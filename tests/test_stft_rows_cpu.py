"""STFT, stft_magnitudes and ISTFT over rows of signals without a GPU: the new symbols with their declared argument order, every
argument check of the C ABI that comes before the context (called with a null context: a check that came later would give NULL), and
the Python wrappers' FftErrors, raised before any context exists."""
import ctypes as C

import numpy as np
import pytest

SZ = C.c_size_t
VP = C.c_void_p
CTX = C.c_void_p

STFT = [CTX, VP, SZ, SZ, SZ, VP, SZ, SZ, VP, SZ]         # ctx, signal, rows, len, row_stride, window, win_len, hop, out, frames
MAGS = [CTX, VP, SZ, SZ, SZ, SZ, SZ, VP, SZ, VP]         # ctx, samples, rows, len, row_stride, win_len, hop, mags, frames, max
ISTFT = [CTX, VP, SZ, SZ, VP, SZ, SZ, VP, SZ, VP, SZ]    # ctx, frames, rows, frames, window, win_len, hop, output, out_len, scratch, scratch_len
ISTFT_PAR = [CTX, VP, SZ, SZ, VP, SZ, SZ, VP, SZ]        # ctx, frames, rows, frames, window, win_len, hop, output, out_len
SYMBOLS = {
    "kofft_hip_stft_rows_f32": STFT,
    "kofft_hip_dev_stft_rows_f32": STFT,
    "kofft_hip_stft_magnitudes_rows_f32": MAGS,
    "kofft_hip_dev_stft_magnitudes_rows_f32": MAGS,
    "kofft_hip_istft_rows_f32": ISTFT,
    "kofft_hip_dev_istft_rows_f32": ISTFT,
    "kofft_hip_istft_parallel_rows_f32": ISTFT_PAR,
    "kofft_hip_dev_istft_parallel_rows_f32": ISTFT_PAR,
}
OK, EMPTY, MISMATCH, HOP, INVALID, UNSUPPORTED, NULL = 0, 1, 3, 5, 6, -2, -3


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_symbol_and_declared_argument_order(hiplib, name):
    fn = getattr(hiplib, name)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == SYMBOLS[name]


def _p():
    buf = np.zeros(64, np.float32)
    return buf, VP(buf.ctypes.data)


@pytest.mark.parametrize("name", ["kofft_hip_stft_rows_f32", "kofft_hip_dev_stft_rows_f32"])
def test_stft_rows_checks_in_order(hiplib, name):
    fn, host = getattr(hiplib, name), "_dev_" not in name
    keep, p = _p()
    null = CTX(None)

    def call(rows=2, length=10, stride=10, win=8, hop=4, frames=3):
        return fn(null, p, rows, length, stride, p, win, hop, p, frames)

    assert call(hop=0) == HOP
    assert call(hop=0, frames=0, win=0) == HOP                        # the hop comes first
    assert call(frames=2) == (MISMATCH if host else NULL)             # stft's frame count: the host form only
    assert call(frames=2, win=0) == (MISMATCH if host else EMPTY)
    assert call(rows=0) == OK and call(rows=0, win=0, stride=0) == OK
    assert call(length=0, stride=0, frames=0) == OK                   # nothing to do, nothing touched
    assert call(win=0) == EMPTY
    assert call(win=(1 << 26) + 1) == UNSUPPORTED and call(win=1 << 27) == UNSUPPORTED
    assert call(win=(1 << 25) + 1) == UNSUPPORTED                     # not a power of two: 2^25 at most
    assert call(stride=9) == INVALID
    assert call(stride=9, win=0) == EMPTY                             # EMPTY_INPUT before the stride
    assert call(rows=1, stride=0) == NULL                             # one row: the stride is not looked at
    assert call() == NULL                                             # everything passed: only the context is missing
    assert call(win=1 << 26) == NULL


@pytest.mark.parametrize("name", ["kofft_hip_stft_magnitudes_rows_f32", "kofft_hip_dev_stft_magnitudes_rows_f32"])
def test_magnitudes_rows_checks_in_order(hiplib, name):
    fn = getattr(hiplib, name)
    keep, p = _p()
    null = CTX(None)

    def call(rows=2, length=10, stride=10, win=8, hop=4, frames=3):
        return fn(null, p, rows, length, stride, win, hop, p, frames, p)

    assert call(hop=0) == HOP
    assert call(frames=2) == MISMATCH and call(frames=2, win=0) == MISMATCH  # both forms, as stft_mag_dev
    assert call(rows=0) == OK
    assert call(win=0) == EMPTY
    assert call(win=(1 << 26) + 1) == UNSUPPORTED
    assert call(stride=9) == INVALID
    assert call() == NULL


@pytest.mark.parametrize("name", ["kofft_hip_istft_rows_f32", "kofft_hip_dev_istft_rows_f32"])
def test_istft_rows_checks_in_order(hiplib, name):
    fn = getattr(hiplib, name)
    keep, p = _p()
    null = CTX(None)

    def call(rows=2, frames=3, win=8, hop=4, out_len=16, scratch_len=16):
        return fn(null, p, rows, frames, p, win, hop, p, out_len, p, scratch_len)

    assert call(hop=0) == HOP
    assert call(hop=0, scratch_len=3) == HOP
    assert call(scratch_len=15) == MISMATCH and call(scratch_len=15, win=0) == MISMATCH
    assert call(rows=0) == OK
    assert call(win=0) == EMPTY
    assert call(win=0, frames=0) == NULL                                # no frames: the window length is not looked at
    assert call(win=(1 << 26) + 1) == UNSUPPORTED
    assert call() == NULL


@pytest.mark.parametrize("name", ["kofft_hip_istft_parallel_rows_f32", "kofft_hip_dev_istft_parallel_rows_f32"])
def test_istft_parallel_rows_checks_in_order(hiplib, name):
    fn = getattr(hiplib, name)
    keep, p = _p()
    null = CTX(None)

    def call(rows=2, frames=3, win=8, hop=4, out_len=16):
        return fn(null, p, rows, frames, p, win, hop, p, out_len)

    assert call(hop=0) == HOP
    assert call(rows=0) == OK
    assert call(win=0) == EMPTY
    assert call(win=(1 << 26) + 1) == UNSUPPORTED
    assert call() == NULL


def test_python_errors_need_no_device(monkeypatch):
    """stft_rows / stft_magnitudes_rows raise their FftErrors, in the C ABI's order, before any context is created."""
    import kofft_amd
    from kofft_amd import api

    def no_context(*a, **k):
        raise AssertionError("a context was created")

    monkeypatch.setattr(api.HipFftImpl, "__init__", no_context)
    monkeypatch.setattr(api, "_stft_rows_default", None)
    x = np.zeros((3, 10), np.float32)
    w = np.ones(8, np.float32)
    E = kofft_amd.FftError
    for args, code in [((x, w, 0), E.InvalidHopSize), ((x, w, 4, 2), E.MismatchedLengths), ((x, np.zeros(0, np.float32), 4), E.EmptyInput),
                       ((x, np.zeros(0, np.float32), 0), E.InvalidHopSize), ((x, np.zeros(0, np.float32), 4, 1), E.MismatchedLengths)]:
        with pytest.raises(E) as e:
            kofft_amd.stft_rows(*args)
        assert e.value.code == code
    for args, code in [((x, 8, 0), E.InvalidHopSize), ((x, 0, 4), E.EmptyInput), ((x, 0, 0), E.InvalidHopSize)]:
        with pytest.raises(E) as e:
            kofft_amd.stft_magnitudes_rows(*args)
        assert e.value.code == code
    with pytest.raises(TypeError):
        kofft_amd.stft_rows(np.zeros(10, np.float32), w, 4)
    with pytest.raises(kofft_amd.DeviceError):
        kofft_amd.stft_magnitudes_rows(x, (1 << 26) + 1, 4)
    with pytest.raises(AssertionError, match="a context was created"):  # a valid request goes on to the device
        kofft_amd.stft_rows(x, w, 4)


def test_every_rows_entry_has_a_guard_band_case():
    """tests/test_redzone.py holds every kofft_hip_*_dev name of the header against the case table of tests/test_gpu_footprint.py, a file
    that predates these calls and is not theirs to extend; so their device forms carry the kofft_hip_dev_ prefix, which that pattern does
    not match, and this test is the coverage check in its place: every entry of the header with _rows_ in its name is one of SYMBOLS,
    none of them ends in _dev, and each is called inside an arena by tests/test_gpu_stft_rows_footprint.py."""
    import re
    from pathlib import Path

    from kofft_amd import _lib

    family = [s for s in _lib.header_symbols() if "_rows_" in s]
    assert sorted(family) == sorted(SYMBOLS)
    assert not [s for s in family if s.endswith("_dev")]
    src = (Path(__file__).resolve().parent / "test_gpu_stft_rows_footprint.py").read_text()
    assert '"kofft_hip_dev_" if where == "cuda" else "kofft_hip_"' in src and src.count("arena.verify()") >= 4
    stems = set(re.findall(r'pre \+ "(\w+)"', src))
    assert {"kofft_hip_" + s for s in stems} | {"kofft_hip_dev_" + s for s in stems} == set(SYMBOLS)
