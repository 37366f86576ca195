"""The modified discrete cosine transform of f32 signals on the device: 2N windowed samples to N real coefficients per
frame at hop N, and back by overlap-add with time-domain alias cancellation, both on one fast DCT-IV (an N/2-point complex transform
between two twiddle multiplications).  Every value is a composition of the reference's operations, bit for bit on every route.

``mdct(x, N)`` takes a 1-D signal or a 2-D [rows, nx] array and returns [rows, frames, N] ([frames, N] for a 1-D signal) unscaled
coefficients; ``imdct(X)`` takes them back to [rows, length] samples.  With a Princen-Bradley window (``sine_window``,
``vorbis_window``, ``kbd_window``: w[i]^2 + w[i + N]^2 = 1) and the defaults -- ``lead = N`` zeros in front, ``frames = ceil(nx / N) +
1``, ``scale = 2 / N`` -- ``imdct(mdct(x, N), length=nx)`` is x.  ``dct4(x)`` is the fast DCT-IV itself on the last axis, any even
length.  ``fft=`` names the f32 HipFftImpl to run on; without one, a context on device 0 is created at the first call and kept.  Shape
and length errors are raised before any context is created."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import api
from .api import FftError, HipFftImpl

__all__ = ["mdct", "imdct", "dct4", "sine_window", "vorbis_window", "kbd_window"]

_default: Optional[HipFftImpl] = None


def _fft(fft: Optional[HipFftImpl]) -> HipFftImpl:
    global _default
    if fft is not None:
        return fft
    if _default is None:
        _default = api.HipFftImpl(np.float32)
    return _default


def _half(N: int) -> int:
    N = int(N)
    if N <= 0:
        raise FftError(FftError.EmptyInput)
    if N % 2:
        raise FftError(FftError.InvalidValue)
    return N


def sine_window(N: int) -> np.ndarray:
    """2N values sin(pi (i + 1/2) / (2N)), computed in float64 and rounded to float32."""
    N = _half(N)
    return np.sin(np.pi * (np.arange(2 * N, dtype=np.float64) + 0.5) / (2 * N)).astype(np.float32)


def vorbis_window(N: int) -> np.ndarray:
    """2N values sin(pi / 2 sin^2(pi (i + 1/2) / (2N))), computed in float64 and rounded to float32."""
    N = _half(N)
    s = np.sin(np.pi * (np.arange(2 * N, dtype=np.float64) + 0.5) / (2 * N))
    return np.sin(0.5 * np.pi * s * s).astype(np.float32)


def kbd_window(N: int, alpha: float = 4.0) -> np.ndarray:
    """The Kaiser-Bessel-derived window of 2N values from a Kaiser window of N + 1 values with beta = pi alpha: w[i] = sqrt(cumsum(k)[i]
    / sum(k)) for i < N, mirrored; computed in float64 and rounded to float32."""
    N = _half(N)
    k = np.kaiser(N + 1, np.pi * float(alpha)).astype(np.float64)
    half = np.sqrt(np.cumsum(k[:N]) / np.sum(k))
    return np.concatenate([half, half[::-1]]).astype(np.float32)


def _window(window, N: int) -> np.ndarray:
    w = sine_window(N) if window is None else np.ascontiguousarray(window, np.float32)
    if w.ndim != 1 or w.size != 2 * N:
        raise FftError(FftError.MismatchedLengths)
    return w


def mdct(x, N: int, window=None, lead: Optional[int] = None, frames: Optional[int] = None, fft: Optional[HipFftImpl] = None) -> np.ndarray:
    """Frame f holds the N coefficients sum_i g[i] cos(pi / N (i + 1/2 + N/2)(k + 1/2)) of g[i] = x[f N + i - lead] w[i], i < 2N, zeros
    outside the signal.  window=None: the sine window; lead=None: N; frames=None: ceil(nx / N) + 1."""
    N = _half(N)
    a = np.ascontiguousarray(x, np.float32)
    if a.ndim not in (1, 2):
        raise TypeError("mdct expects a 1-D signal or a 2-D [rows, nx] array")
    w = _window(window, N)
    nx = a.shape[-1]
    if nx == 0:
        raise FftError(FftError.EmptyInput)
    if lead is not None and not 0 <= int(lead) < 2 * N:
        raise FftError(FftError.InvalidValue)
    if frames is not None and int(frames) < 0:
        raise ValueError("frames is usize: it cannot be negative")
    out = _fft(fft).mdct_rows(a.reshape(-1, nx), w, lead, frames)
    return out.reshape(a.shape[:-1] + out.shape[1:])


def imdct(X, window=None, length: Optional[int] = None, scale: Optional[float] = None, fft: Optional[HipFftImpl] = None) -> np.ndarray:
    """The inverse of mdct with its defaults: samples N .. N + length of the overlap-added frames (the ``lead = N`` zeros dropped),
    length=None: (frames - 1) N, every sample two frames cover.  window=None: the sine window; scale=None: 2 / N."""
    a = np.ascontiguousarray(X, np.float32)
    if a.ndim not in (2, 3):
        raise TypeError("imdct expects a 2-D [frames, N] or a 3-D [rows, frames, N] array")
    frames, N = a.shape[-2], _half(a.shape[-1])
    w = _window(window, N)
    full = (frames + 1) * N
    count = max(full - 2 * N, 0) if length is None else int(length)
    if count < 0:
        raise ValueError("length is usize: it cannot be negative")
    if N + count > full:
        raise FftError(FftError.MismatchedLengths)
    out = _fft(fft).imdct_rows(a.reshape(-1, frames, N), w, scale, N, count)
    return out.reshape(a.shape[:-2] + (count,))


def dct4(x, fft: Optional[HipFftImpl] = None) -> np.ndarray:
    """The fast DCT-IV over the last axis (an even length): sum_i x[i] cos(pi / n (i + 1/2)(k + 1/2)), unscaled.  kofft_amd.dct.dct4 is
    the reference's direct sum of the same values; the two differ in the last bits."""
    if np.ndim(x) == 0:
        raise TypeError("dct4 expects an array of at least one axis")
    a = np.ascontiguousarray(x, np.float32)
    n = _half(a.shape[-1])
    out = _fft(fft).dct4_fast_batch(a.reshape(-1, n))
    return out.reshape(a.shape)
