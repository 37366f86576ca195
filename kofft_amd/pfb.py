"""The polyphase filter bank of f32 signals on the device: a prototype filter of ``T * channels`` taps folded onto a
``channels``-point transform at hop ``hop`` (a weighted-overlap-add channelizer), and its synthesis, the inverse transforms overlap-added
under a synthesis filter.  Every value is a composition of the reference's operations, bit for bit on every route.

``analysis(x, taps, channels)`` takes a 1-D signal or a 2-D [rows, nx] array and returns [rows, frames, bins] complex64 ([frames, bins]
for a 1-D signal); ``synthesis(spec, taps, channels, hop)`` takes such frames back to [rows, length] samples.  ``prototype(channels,
taps_per_channel)`` designs the usual sinc x Kaiser analysis filter; ``reconstruction(h, g, channels, hop)`` says whether a pair of
filters reconstructs: it returns ``(c, worst)``, and where ``worst`` is (close to) zero, ``synthesis(analysis(x, h, M, D, lead=nh - D),
g, M, D, scale=1 / c, out_first=nh - D, out_len=nx)`` is x.  The sine window with ``T = 1`` and ``hop = channels / 2`` is such a pair;
a sinc x Kaiser prototype used on both sides is not.  ``fft=`` names the f32 HipFftImpl to run on; without one, a context on device 0
is created at the first call and kept.  Shape and length errors are raised before any context is created."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np

from . import _lib, api
from .api import FftError, HipFftImpl

__all__ = ["analysis", "synthesis", "prototype", "reconstruction"]

_default: Optional[HipFftImpl] = None


def _fft(fft: Optional[HipFftImpl]) -> HipFftImpl:
    global _default
    if fft is not None:
        return fft
    if _default is None:
        _default = api.HipFftImpl(np.float32)
    return _default


def _raise(rc: int, what: str) -> None:
    if rc > 0:
        raise FftError(rc)
    if rc < 0:
        raise api.DeviceError(rc, what)


def _shape(taps, channels: int, hop) -> Tuple[np.ndarray, int, int]:
    """The checks both directions share, in the C entries' order: (taps, M, D)."""
    h = np.ascontiguousarray(taps, np.float32)
    if h.ndim != 1:
        raise TypeError("taps must be 1-D")
    M = int(channels)
    if M < 0:
        raise ValueError("channels is usize: it cannot be negative")
    if M == 0 or h.size == 0:
        raise FftError(FftError.EmptyInput)
    if h.size % M:
        raise FftError(FftError.InvalidValue)
    D = M if hop is None else int(hop)
    if D < 0:
        raise ValueError("hop is usize: it cannot be negative")
    if D == 0:
        raise FftError(FftError.InvalidHopSize)
    return h, M, D


def prototype(channels: int, taps_per_channel: int, beta: float = 5.0) -> np.ndarray:
    """kofft_hip_pfb_taps_f32: the nh = taps_per_channel * channels values sinc((i - (nh - 1) / 2) / channels) under a Kaiser window of
    ``beta``, normalised to unit sum; computed in double and rounded to float32 once.  No device."""
    M, T = int(channels), int(taps_per_channel)
    if M < 0 or T < 0:
        raise ValueError("sizes are usize: they cannot be negative")
    out = np.empty(M * T, np.float32)
    _raise(_lib.load().kofft_hip_pfb_taps_f32(M, T, float(beta), C.c_void_p(out.ctypes.data)), "kofft_hip_pfb_taps_f32")
    return out


def reconstruction(h, g, channels: int, hop: int) -> Tuple[float, float]:
    """kofft_hip_pfb_reconstruction: (c, worst) of the condition sum_f g[n_f] h[n_f + q channels] = c delta[q], n_f = p - f hop, evaluated
    in double over every p mod hop and q; c is the q = 0 sum at p = 0, worst the largest deviation.  No device."""
    ha, M, D = _shape(h, channels, hop)
    ga = np.ascontiguousarray(g, np.float32)
    if ga.shape != ha.shape:
        raise FftError(FftError.MismatchedLengths)
    c, worst = C.c_double(0.0), C.c_double(0.0)
    _raise(_lib.load().kofft_hip_pfb_reconstruction(C.c_void_p(ha.ctypes.data), C.c_void_p(ga.ctypes.data), ha.size, M, D, C.byref(c),
                                                    C.byref(worst)), "kofft_hip_pfb_reconstruction")
    return c.value, worst.value


def analysis(x, taps, channels: int, hop: Optional[int] = None, lead: int = 0, frames: Optional[int] = None, onesided: bool = True,
             fft: Optional[HipFftImpl] = None) -> np.ndarray:
    """Frame f holds bins k < bins of Z[k] = sum_i taps[i] x[f hop + i - lead] exp(-2 pi i k i / channels), zeros outside the signal.
    hop=None: channels (critically sampled); frames=None: ceil((nx + lead) / hop), every frame that reaches a sample; onesided:
    channels // 2 + 1 bins, otherwise all of them."""
    a = np.ascontiguousarray(x, np.float32)
    if a.ndim not in (1, 2):
        raise TypeError("analysis expects a 1-D signal or a 2-D [rows, nx] array")
    h, M, D = _shape(taps, channels, hop)
    nx = a.shape[-1]
    if nx == 0:
        raise FftError(FftError.EmptyInput)
    lead = int(lead)
    if not 0 <= lead < h.size:
        raise FftError(FftError.InvalidValue)
    frames = -(-(nx + lead) // D) if frames is None else int(frames)
    if frames < 0:
        raise ValueError("frames is usize: it cannot be negative")
    bins = M // 2 + 1 if onesided else M
    out = _fft(fft).pfb_analysis(a.reshape(-1, nx), h, M, D, lead, frames, bins)
    return out.reshape(a.shape[:-1] + out.shape[1:])


def synthesis(spec, taps, channels: int, hop: int, scale: float = 1.0, out_first: int = 0, out_len: Optional[int] = None,
              fft: Optional[HipFftImpl] = None) -> np.ndarray:
    """Samples out_first .. out_first + out_len of the (frames - 1) hop + nh overlap-added samples per row (out_len=None: up to the end):
    each the sum over its covering frames f of taps[p - f hop] * ifft(F_f)[(p - f hop) mod channels].re, times ``scale``.  The last
    axis of spec holds ``channels`` bins or the one-sided ``channels // 2 + 1`` (channels even)."""
    a = np.ascontiguousarray(spec, np.complex64)
    if a.ndim not in (2, 3):
        raise TypeError("synthesis expects a 2-D [frames, bins] or a 3-D [rows, frames, bins] array")
    g, M, D = _shape(taps, channels, hop)
    frames, bins = a.shape[-2], a.shape[-1]
    if bins != M and not (M % 2 == 0 and bins == M // 2 + 1):
        raise FftError(FftError.InvalidValue)
    first = int(out_first)
    if first < 0 or (out_len is not None and int(out_len) < 0):
        raise ValueError("out_first and out_len are usize: they cannot be negative")
    full = (frames - 1) * D + g.size if frames else 0
    count = max(full - first, 0) if out_len is None else int(out_len)
    if frames and first + count > full:
        raise FftError(FftError.MismatchedLengths)
    out = _fft(fft).pfb_synthesis(a.reshape(-1, frames, bins), g, M, D, scale, first, count)
    return out.reshape(a.shape[:-2] + (count,))
