"""The one-sided STFT and its inverse without a GPU: the four symbols with their declared argument order, every argument
check of the C ABI that comes before the context (called with a null context: a check that came later would give NULL), the Python free
functions' errors raised before any context exists, the NumPy restatement of the Hermitian completion that the GPU tests use as their
reference, and the round-trip bound of tests/test_gpu_stft_onesided.py confirmed with the oracle alone on the signals that test uses."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits_equal
from onesided_ref import ROUND_TRIPS, bins, complete, round_trip_errors, round_trip_signal

SZ = C.c_size_t
VP = C.c_void_p
CTX = C.c_void_p

STFT = [CTX, VP, SZ, SZ, SZ, VP, SZ, SZ, VP, SZ]  # ctx, signal, rows, len, row_stride, window, win_len, hop, out, frames
ISTFT = [CTX, VP, SZ, SZ, VP, SZ, SZ, VP, SZ]     # ctx, half, rows, frames, window, win_len, hop, output, out_len
SYMBOLS = {
    "kofft_hip_stft_onesided_f32": STFT,
    "kofft_hip_dev_stft_onesided_f32": STFT,
    "kofft_hip_istft_onesided_f32": ISTFT,
    "kofft_hip_dev_istft_onesided_f32": ISTFT,
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


@pytest.mark.parametrize("name", ["kofft_hip_stft_onesided_f32", "kofft_hip_dev_stft_onesided_f32"])
def test_stft_onesided_checks_in_order(hiplib, name):
    """stft_rows_check's checks in its order (tests/test_stft_rows_cpu.py holds the rows call to the same list)."""
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
    assert call(rows=1 << 40, frames=1 << 30, length=1 << 31, stride=1 << 31, win=2) == UNSUPPORTED  # rows * frames * bins overflows
    assert call() == NULL                                             # everything passed: only the context is missing
    assert call(win=1 << 26) == NULL and call(win=1) == NULL and call(win=3) == NULL


@pytest.mark.parametrize("name", ["kofft_hip_istft_onesided_f32", "kofft_hip_dev_istft_onesided_f32"])
def test_istft_onesided_checks_in_order(hiplib, name):
    """istft_rows_check(mode 2)'s checks in its order."""
    fn = getattr(hiplib, name)
    keep, p = _p()
    null = CTX(None)

    def call(rows=2, frames=3, win=8, hop=4, out_len=16):
        return fn(null, p, rows, frames, p, win, hop, p, out_len)

    assert call(hop=0) == HOP
    assert call(hop=0, win=0) == HOP and call(hop=0, rows=0) == HOP
    assert call(rows=0) == OK and call(rows=0, win=0) == OK
    assert call(win=0) == EMPTY
    assert call(win=0, frames=0) == NULL                                # no frames: the window length is not looked at
    assert call(win=(1 << 26) + 1) == UNSUPPORTED and call(win=(1 << 25) + 1) == UNSUPPORTED
    assert call(rows=1 << 40, frames=1 << 30) == UNSUPPORTED
    assert call() == NULL and call(win=1) == NULL and call(win=15) == NULL


def test_python_errors_need_no_device(monkeypatch):
    """stft_onesided / istft_onesided raise their FftErrors, in the C ABI's order, before any context is created."""
    import kofft_amd
    from kofft_amd import api

    def no_context(*a, **k):
        raise AssertionError("a context was created")

    monkeypatch.setattr(api.HipFftImpl, "__init__", no_context)
    monkeypatch.setattr(api, "_stft_rows_default", None)
    x = np.zeros((3, 10), np.float32)
    w = np.ones(8, np.float32)
    none = np.zeros(0, np.float32)
    E = kofft_amd.FftError
    for args, code in [((x, w, 0), E.InvalidHopSize), ((x, w, 4, 2), E.MismatchedLengths), ((x, none, 4), E.EmptyInput),
                       ((x, none, 0), E.InvalidHopSize), ((x, none, 4, 1), E.MismatchedLengths)]:
        with pytest.raises(E) as e:
            kofft_amd.stft_onesided(*args)
        assert e.value.code == code
    with pytest.raises(TypeError):
        kofft_amd.stft_onesided(np.zeros(10, np.float32), w, 4)
    with pytest.raises(kofft_amd.DeviceError):
        kofft_amd.stft_onesided(x, np.zeros((1 << 25) + 1, np.float32), 4)
    with pytest.raises(AssertionError, match="a context was created"):  # a valid request goes on to the device
        kofft_amd.stft_onesided(x, w, 4)
    half = np.zeros((3, 4, 5), np.complex64)
    out = np.zeros((3, 20), np.float32)
    for args, code in [((half, w, 0, out), E.InvalidHopSize), ((half, none, 0, out), E.InvalidHopSize),
                       ((half, np.ones(10, np.float32), 4, out), E.MismatchedLengths),  # 5 bins are a window of 8 or 9, not 10
                       ((half, w, 4, np.zeros((2, 20), np.float32)), E.MismatchedLengths),
                       ((np.zeros((3, 4, 1), np.complex64), none, 4, out), E.EmptyInput)]:
        with pytest.raises(E) as e:
            kofft_amd.istft_onesided(*args)
        assert e.value.code == code
    with pytest.raises(TypeError):
        kofft_amd.istft_onesided(np.zeros((3, 4, 5), np.complex128), w, 4, out)
    with pytest.raises(AssertionError, match="a context was created"):
        kofft_amd.istft_onesided(half, w, 4, out)


def test_every_onesided_entry_has_a_guard_band_case():
    """Every entry of the header with `onesided` in its name is one of SYMBOLS; none of them ends in _dev (the pattern of
    tests/test_redzone.py) or contains _rows_ (the family of tests/test_stft_rows_cpu.py); each is called inside an arena by
    tests/test_gpu_stft_onesided_footprint.py."""
    import re
    from pathlib import Path

    from kofft_amd import _lib

    family = [s for s in _lib.header_symbols() if "onesided" in s]
    assert sorted(family) == sorted(SYMBOLS)
    assert not [s for s in family if s.endswith("_dev") or "_rows_" in s]
    assert set(SYMBOLS) <= set(_lib.SIGNATURES)
    src = (Path(__file__).resolve().parent / "test_gpu_stft_onesided_footprint.py").read_text()
    assert '"kofft_hip_dev_" if where == "cuda" else "kofft_hip_"' in src and src.count("arena.verify()") >= 2
    stems = set(re.findall(r'pre \+ "(\w+)"', src))
    assert {"kofft_hip_" + s for s in stems} | {"kofft_hip_dev_" + s for s in stems} == set(SYMBOLS)


def _c(*pairs):
    return np.array([complex(re, im) for re, im in pairs], np.complex64)


# n -> (half, the completed frame written out by hand)
COMPLETIONS = {
    1: (_c((1, 2)), _c((1, 2))),
    2: (_c((1, 2), (3, 4)), _c((1, 2), (3, 4))),
    3: (_c((1, 2), (3, 4)), _c((1, 2), (3, 4), (3, -4))),
    8: (_c((1, 2), (3, 4), (5, -6), (7, 0.0), (9, 10)), _c((1, 2), (3, 4), (5, -6), (7, 0.0), (9, 10), (7, -0.0), (5, 6), (3, -4))),
    15: (_c(*[(k + 1, 0.5 * k - 2) for k in range(8)]),
         _c(*([(k + 1, 0.5 * k - 2) for k in range(8)] + [(k + 1, -(0.5 * k - 2)) for k in range(7, 0, -1)]))),
}


@pytest.mark.parametrize("n", sorted(COMPLETIONS))
def test_numpy_restatement_of_the_hermitian_completion(n):
    """F[k] = H[k] for k < K, (H[n - k].re, -H[n - k].im) for K <= k < n; the imaginary parts of H[0] and H[n / 2] are used as given
    (n = 8: H[4] = 9 + 10i stays), and negating +0 gives -0 (n = 8: H[3])."""
    half, want = COMPLETIONS[n]
    assert bins(n) == half.size and want.size == n
    assert bits_equal(complete(half, n), want)
    twice = lambda a: (a.view(np.float32) * np.float32(2)).view(np.complex64)  # (on the parts: a complex product would turn -0 into +0)
    batch = np.stack([half, twice(half)]).reshape(2, 1, -1)
    assert bits_equal(complete(batch, n), np.stack([want, twice(want)]).reshape(2, 1, -1))
    with pytest.raises(ValueError):
        complete(np.zeros(bins(n) + 1, np.complex64), n)


def test_completion_of_a_real_signals_spectrum_is_the_spectrum(oracle):
    """For real input the oracle's upper bins are the mirror of the lower ones up to rounding, and exactly so at n = 8."""
    rng = np.random.default_rng(66001)
    x = rng.uniform(-1, 1, 40).astype(np.float32)
    win = rng.uniform(0.1, 1, 8).astype(np.float32)
    spec = oracle.stft(x, win, 4, 10)
    assert np.allclose(complete(spec[:, :5], 8), spec, atol=1e-6)


@pytest.mark.parametrize("win_len,hop,seed", ROUND_TRIPS)
def test_round_trip_bound_holds_with_the_oracle_alone(oracle, win_len, hop, seed):
    """The GPU test asserts error(one-sided trip) <= 2 x error(full trip) on these very signals; here both trips are the oracle's."""
    import kofft_amd

    one, full = round_trip_errors(oracle, round_trip_signal(win_len, hop, seed), kofft_amd.hann(win_len), hop)
    print(f"win {win_len} hop {hop}: one-sided {one:.3e} full {full:.3e} ratio {one / full:.3f}")
    assert full > 0 and one <= 2 * full
