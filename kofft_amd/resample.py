"""Polyphase sample-rate conversion of f32 rows on the device: an FIR filter applied between an up-sampling by ``up``
and a down-sampling by ``down`` without the zero-stuffed signal ever existing.  Output m of a row sits at up-sampled time
t = t0 + m * down and is the sum of h[p + j * up] * x[i0 - j], p = t mod up, i0 = t div up, over ascending j in one f32 accumulator,
un-fused, the terms whose sample does not exist skipped: bit for bit the definition in include/kofft_hip.h on every route.

``upfirdn(h, x, up, down)`` is scipy.signal.upfirdn: t0 = 0 and ceil(((nx - 1) * up + nh) / down) outputs.  ``resample_poly(x, up,
down)`` is scipy.signal.resample_poly with its default filter and padtype "constant": up / down reduced by their gcd, a float32 copy
at 1 / 1, t0 = (nh - 1) // 2 and ceil(nx * up / down) outputs.  ``taps=`` replaces the designed filter by the caller's, **used as
given** (scipy multiplies a window passed as an array by ``up``; here that product is the caller's).  ``design_taps`` is the filter
resample_poly designs: a Kaiser-windowed sinc of 2 * zeros * max(up, down) + 1 taps, normalised to unit sum and multiplied by up.

``x`` is a 1-D signal or a 2-D [rows, nx] array; the result has the same rank.  ``fft=`` names the f32 HipFftImpl to run on; without
one, a context on device 0 is created at the first call and kept.  Shape and value errors are raised before any context is created."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np

from . import _lib, api
from .api import FftError, HipFftImpl

__all__ = ["upfirdn", "resample_poly", "design_taps", "route"]

_default: Optional[HipFftImpl] = None


def _raise(rc: int, what: str):
    if rc > 0:
        raise FftError(rc)
    if rc < 0:
        raise api.DeviceError(rc, what)


def _rates(up, down):
    up, down = int(up), int(down)
    if up < 0 or down < 0:
        raise ValueError("up and down are usize: they cannot be negative")
    if up == 0 or down == 0:
        raise FftError(FftError.InvalidValue)
    return up, down


def design_taps(up: int, down: int, zeros: int = 10, beta: float = 5.0) -> np.ndarray:
    """kofft_hip_resample_taps_f32: scipy.signal.firwin(2 * zeros * max(up, down) + 1, 1 / max(up, down), window=("kaiser", beta)) * up,
    computed in double and rounded to float32 once.  No device."""
    if int(up) < 0 or int(down) < 0 or int(zeros) < 0:
        raise ValueError("up, down and zeros are usize: they cannot be negative")
    lib = _lib.load()
    nh = C.c_size_t()
    _raise(lib.kofft_hip_resample_taps_f32(int(up), int(down), int(zeros), float(beta), None, C.byref(nh)), "kofft_hip_resample_taps_f32")
    taps = np.empty(nh.value, np.float32)
    _raise(lib.kofft_hip_resample_taps_f32(int(up), int(down), int(zeros), float(beta), C.c_void_p(taps.ctypes.data), C.byref(nh)),
           "kofft_hip_resample_taps_f32")
    return taps


def route(nh: int, up: int, down: int) -> int:
    """kofft_hip_resample_route: 1 where a default context runs the tiled kernel, 0 where the plain one.  No device."""
    if min(int(nh), int(up), int(down)) < 0:
        raise ValueError("nh, up and down are usize: they cannot be negative")
    r = C.c_int()
    _raise(_lib.load().kofft_hip_resample_route(int(nh), int(up), int(down), C.byref(r)), "kofft_hip_resample_route")
    return int(r.value)


def _inputs(x, h):
    a = np.ascontiguousarray(x, np.float32)
    taps = np.ascontiguousarray(h, np.float32)
    if a.ndim not in (1, 2) or taps.ndim != 1:
        raise TypeError("expected a 1-D signal or a 2-D [rows, nx] array, and 1-D [nh] taps")
    if a.shape[-1] == 0 or taps.shape[0] == 0:
        raise FftError(FftError.EmptyInput)
    return a, taps


def _run(a, taps, up, down, t0, out_len, fft):
    global _default
    if fft is None:
        if _default is None:
            _default = api.HipFftImpl(np.float32)
        fft = _default
    nx = a.shape[-1]
    full_up = (nx - 1) * up + taps.shape[0]
    have = min(out_len, max(-(-(full_up - t0) // down), 0))  # the outputs that begin inside the full result; the rest are +0
    out = fft.resample_rows(a.reshape(-1, nx), taps, up, down, t0, have)
    if have < out_len:
        out = np.concatenate([out, np.zeros((out.shape[0], out_len - have), np.float32)], axis=1)
    return out.reshape(a.shape[:-1] + (out_len,))


def upfirdn(h, x, up: int = 1, down: int = 1, fft: Optional[HipFftImpl] = None) -> np.ndarray:
    """scipy.signal.upfirdn(h, x, up, down) of every row, in f32: ceil(((nx - 1) * up + nh) / down) values per row."""
    up, down = _rates(up, down)
    a, taps = _inputs(x, h)
    full_up = (a.shape[-1] - 1) * up + taps.shape[0]
    return _run(a, taps, up, down, 0, -(-full_up // down), fft)


def resample_poly(x, up: int, down: int, taps=None, zeros: int = 10, beta: float = 5.0, fft: Optional[HipFftImpl] = None) -> np.ndarray:
    """scipy.signal.resample_poly(x, up, down, window=("kaiser", beta)) of every row, in f32: ceil(nx * up / down) values per row, rows
    ending in silence.  ``taps``: the filter to use instead of ``design_taps(up, down, zeros, beta)`` (of the reduced rates), as given."""
    up, down = _rates(up, down)
    g = math.gcd(up, down)
    up, down = up // g, down // g
    a = np.ascontiguousarray(x, np.float32)
    if a.ndim not in (1, 2):
        raise TypeError("expected a 1-D signal or a 2-D [rows, nx] array")
    if up == 1 and down == 1:
        return a.copy()
    h = design_taps(up, down, zeros, beta) if taps is None else taps
    a, h = _inputs(a, h)
    return _run(a, h, up, down, (h.shape[0] - 1) // 2, -(-a.shape[-1] * up // down), fft)
