"""Welch power spectral densities and cross-spectral densities of f32 signals on the device: the average over the
whole segments of a signal of |X[k]|^2, or of conj(X[k]) Y[k], X and Y the one-sided STFT frames the library writes.  No frame ever
leaves the device and the result is defined bit for bit: the summation order is part of the C contract (include/kofft_hip.h).

``welch`` / ``csd`` take a 1-D signal or a 2-D [rows, len] array and return ``(freqs, pxx)``: ``freqs`` the win_len // 2 + 1 bin
frequencies in float64, ``pxx`` float32 (``csd``: complex64) of the same rank as ``x``.  ``hop`` None is win_len // 2, ``window``
None the library's window::hann(win_len); ``scaling`` is scipy's "density" (V^2 / Hz) or "spectrum" (V^2); ``onesided_double``
doubles the interior bins, as scipy does for a one-sided spectrum.

There is NO detrending: scipy.signal.welch's default ``detrend="constant"`` removes every segment's mean first and differs, compare
with ``detrend=False``.  The average is the mean; there is no median.  Only whole segments count: ``segments(len, win_len, hop)``.
Coherence and transfer functions are compositions of three calls: |csd(x, y)|^2 / (welch(x) welch(y)) and csd(x, y) / welch(x).

``fft=`` names the f32 HipFftImpl to run on; without one, a context on device 0 is created at the first call and kept.  Shape, size
and scaling errors are raised before any context is created."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib, api
from .api import FftError, HipFftImpl

__all__ = ["welch", "csd", "segments", "scale"]

_default: Optional[HipFftImpl] = None
_SCALINGS = {"density": 0, "spectrum": 1}


def segments(length: int, win_len: int, hop: int) -> int:
    """The whole segments of win_len samples, hop apart, in a signal of ``length`` samples: (length - win_len) // hop + 1, or 0 when
    the signal is shorter than one segment."""
    length, win_len, hop = int(length), int(win_len), int(hop)
    if length < 0 or win_len < 0 or hop < 0:
        raise ValueError("length, win_len and hop are usize: they cannot be negative")
    if hop == 0:
        raise FftError(FftError.InvalidHopSize)
    return 0 if length < win_len else (length - win_len) // hop + 1


def scale(window, win_len: int, fs: float, frames: int, scaling: str = "density") -> float:
    """kofft_hip_welch_scale_f32: 1 / (fs * sum w^2 * frames) ("density") or 1 / ((sum w)^2 * frames) ("spectrum"), the sums ascending
    in double, rounded to f32 once; ``window`` None is window::hann(win_len).  Needs no device."""
    if scaling not in _SCALINGS:
        raise ValueError('scaling must be "density" or "spectrum"')
    win = None if window is None else np.ascontiguousarray(window, np.float32)
    if win is not None and (win.ndim != 1 or win.size != int(win_len)):
        raise TypeError("the window must be 1-D with win_len values")
    out = C.c_float()
    rc = _lib.load().kofft_hip_welch_scale_f32(None if win is None else win.ctypes.data_as(C.c_void_p), int(win_len), float(fs), int(frames),
                                              _SCALINGS[scaling], C.byref(out))
    if rc > 0:
        raise FftError(rc)
    if rc < 0:
        raise api.DeviceError(rc, "kofft_hip_welch_scale_f32")
    return float(out.value)


def _run(x, y, win_len, hop, window, fs, scaling, onesided_double, fft):
    global _default
    a = np.ascontiguousarray(x, np.float32)
    b = None if y is None else np.ascontiguousarray(y, np.float32)
    if a.ndim not in (1, 2) or (b is not None and b.shape != a.shape):
        raise TypeError("welch / csd expect a 1-D signal or a 2-D [rows, len] array (csd: two of one shape)")
    if scaling not in _SCALINGS:
        raise ValueError('scaling must be "density" or "spectrum"')
    win_len = int(win_len)
    if win_len < 0:
        raise ValueError("win_len is a usize: it cannot be negative")
    if win_len == 0:
        raise FftError(FftError.EmptyInput)
    hop = win_len // 2 if hop is None else int(hop)
    length = a.shape[-1]
    frames = segments(length, win_len, hop)  # (hop == 0: InvalidHopSize)
    if frames == 0:
        raise FftError(FftError.MismatchedLengths)  # the signal is shorter than one segment
    if not float(fs) > 0.0:
        raise FftError(FftError.InvalidValue)
    rows = a.reshape(-1, length)
    sig, other, win = api._welch_args(rows, None if b is None else b.reshape(-1, length), win_len, hop, frames, window)
    s = scale(win, win_len, fs, frames, scaling)
    if fft is None:
        if _default is None:
            _default = api.HipFftImpl(np.float32)
        fft = _default
    if other is None:
        out = fft.welch_rows(sig, win_len, hop, frames, win, s, bool(onesided_double))
    else:
        out = fft.csd_rows(sig, other, win_len, hop, frames, win, s, bool(onesided_double))
    freqs = np.arange(win_len // 2 + 1, dtype=np.float64) * (float(fs) / win_len)
    return freqs, out.reshape(a.shape[:-1] + (win_len // 2 + 1,))


def welch(x, win_len: int, hop: Optional[int] = None, window=None, fs: float = 1.0, scaling: str = "density", onesided_double: bool = True,
          fft: Optional[HipFftImpl] = None):
    """(freqs, pxx): scipy.signal.welch(x, fs, window, nperseg=win_len, noverlap=win_len - hop, detrend=False, scaling=scaling) of
    every row, in f32.  No detrending (scipy's default detrend="constant" differs)."""
    return _run(x, None, win_len, hop, window, fs, scaling, onesided_double, fft)


def csd(x, y, win_len: int, hop: Optional[int] = None, window=None, fs: float = 1.0, scaling: str = "density", onesided_double: bool = True,
        fft: Optional[HipFftImpl] = None):
    """(freqs, pxy): scipy.signal.csd(x, y, ..., detrend=False) of every row, conj(X) Y, in f32.  No detrending."""
    return _run(x, y, win_len, hop, window, fs, scaling, onesided_double, fft)
