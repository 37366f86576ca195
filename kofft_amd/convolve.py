"""FFT convolution and cross-correlation of f32 signals on the device by overlap-save: frames of ``block`` samples at
hop ``block - nh + 1``, each transformed, multiplied by the filter's spectrum and transformed back, the last ``hop`` real parts of
every frame kept.  Every value is a composition of the reference's operations (fft, Complex::mul, ifft), bit for bit; the bits depend
on ``block``.

``convolve`` / ``correlate`` take a 1-D signal or a 2-D [rows, nx] array and 1-D [nh] taps (all rows) or 2-D [rows, nh] taps (one
filter per row), and return float32 of the same rank as ``x``.  ``mode`` is numpy's: "full" (nx + nh - 1 values), "same" (nx values
from (nh - 1) // 2) or "valid" (nx - nh + 1 values, nx >= nh).  ``correlate(x, h)`` is ``convolve(x, reverse(h))``:
numpy.correlate(x, h) for real data.  ``block`` is the power-of-two transform length, at least nh; None takes ``default_block(nx, nh)``.
``fft=`` names the f32 HipFftImpl to run on; without one, a context on device 0 is created at the first call and kept.  Shape, mode
and block errors are raised before any context is created.

``convolve_bank`` / ``correlate_bank`` apply every filter of a 2-D [filters, nh] bank, float32 or complex64, to every
row: each frame is loaded and transformed once for the whole bank.  The result is [rows, filters, count] ([filters, count] for a 1-D
signal): float32 real parts (``out="real"``), complex64 values ("complex") or float32 magnitudes ("magnitude").  ``correlate_bank``
reverses the taps and conjugates complex ones, as numpy.correlate does."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib, api
from .api import FftError, HipFftImpl

__all__ = ["convolve", "correlate", "convolve_bank", "correlate_bank", "default_block"]

_default: Optional[HipFftImpl] = None


def default_block(nx: int, nh: int) -> int:
    """The block a call without one runs with (kofft_hip_convolve_block): p = next_pow2(nx + nh - 1) up to 4096; on longer rows 2048
    for nh <= 1024, 4096 for nh <= 2048, then min(p, next_pow2(2 nh))."""
    if int(nx) < 0 or int(nh) < 0:
        raise ValueError("nx and nh are usize: they cannot be negative")
    block = C.c_size_t()
    rc = _lib.load().kofft_hip_convolve_block(int(nx), int(nh), C.byref(block))
    if rc > 0:
        raise FftError(rc)
    if rc < 0:
        raise api.DeviceError(rc, "kofft_hip_convolve_block")
    return int(block.value)


def _window(mode: str, nx: int, nh: int):
    """(first, count) of numpy's mode inside the full result of nx + nh - 1 values."""
    if mode == "full":
        return 0, nx + nh - 1
    if mode == "same":
        return (nh - 1) // 2, nx
    if nx < nh:
        raise FftError(FftError.MismatchedLengths)
    return nh - 1, nx - nh + 1


def _run(x, h, mode: str, block: Optional[int], fft: Optional[HipFftImpl], correlate_: bool) -> np.ndarray:
    global _default
    a = np.ascontiguousarray(x, np.float32)
    taps = np.ascontiguousarray(h, np.float32)
    if a.ndim not in (1, 2) or taps.ndim not in (1, 2):
        raise TypeError("convolve expects a 1-D signal or a 2-D [rows, nx] array, and 1-D [nh] or 2-D [rows, nh] taps")
    if mode not in ("full", "same", "valid"):
        raise ValueError('mode must be "full", "same" or "valid"')
    nx, nh = a.shape[-1], taps.shape[-1]
    if nx == 0 or nh == 0:
        raise FftError(FftError.EmptyInput)
    rows_x = a.reshape(-1, nx)
    rows = rows_x.shape[0]
    if taps.ndim == 2 and taps.shape[0] != rows:
        raise FftError(FftError.MismatchedLengths)
    if block is not None:
        block = int(block)
        if block <= 0 or block & (block - 1):
            raise FftError(FftError.NonPowerOfTwoNoStd)
        if block < nh:
            raise FftError(FftError.MismatchedLengths)
    first, count = _window(mode, nx, nh)
    if fft is None:
        if _default is None:
            _default = api.HipFftImpl(np.float32)
        fft = _default
    out = fft.convolve_rows(rows_x, taps, block, correlate_, first, count)
    return out.reshape(a.shape[:-1] + (count,))


def convolve(x, h, mode: str = "full", block: Optional[int] = None, fft: Optional[HipFftImpl] = None) -> np.ndarray:
    """numpy.convolve(x, h, mode) of every row, in f32 by overlap-save."""
    return _run(x, h, mode, block, fft, False)


def correlate(x, h, mode: str = "full", block: Optional[int] = None, fft: Optional[HipFftImpl] = None) -> np.ndarray:
    """numpy.correlate(x, h, mode) of every row (real data: the taps reversed, not conjugated), in f32 by overlap-save.  The modes
    are the windows of convolve(x, reverse(h)): "same" starts at (nh - 1) // 2 of the full result."""
    return _run(x, h, mode, block, fft, True)


def _run_bank(x, h, mode: str, block: Optional[int], out: str, fft: Optional[HipFftImpl], correlate_: bool) -> np.ndarray:
    global _default
    a = np.ascontiguousarray(x, np.float32)
    taps = np.asarray(h)
    taps = np.ascontiguousarray(taps, np.complex64 if np.iscomplexobj(taps) else np.float32)
    if a.ndim not in (1, 2) or taps.ndim != 2:
        raise TypeError("convolve_bank expects a 1-D signal or a 2-D [rows, nx] array, and 2-D [filters, nh] taps")
    if mode not in ("full", "same", "valid"):
        raise ValueError('mode must be "full", "same" or "valid"')
    if out not in HipFftImpl.BANK_KINDS:
        raise ValueError('out must be "real", "complex" or "magnitude"')
    nx, nh = a.shape[-1], taps.shape[-1]
    if nx == 0 or nh == 0:
        raise FftError(FftError.EmptyInput)
    if block is not None:
        block = int(block)
        if block <= 0 or block & (block - 1):
            raise FftError(FftError.NonPowerOfTwoNoStd)
        if block < nh:
            raise FftError(FftError.MismatchedLengths)
    first, count = _window(mode, nx, nh)
    if fft is None:
        if _default is None:
            _default = api.HipFftImpl(np.float32)
        fft = _default
    res = fft.convolve_bank_rows(a.reshape(-1, nx), taps, block, correlate_, first, count, out)
    return res.reshape(a.shape[:-1] + (taps.shape[0], count))


def convolve_bank(x, h, mode: str = "full", block: Optional[int] = None, out: str = "real", fft: Optional[HipFftImpl] = None) -> np.ndarray:
    """numpy.convolve(x[r], h[f], mode) for every row r and every filter f of the [filters, nh] bank h, in f32 by overlap-save."""
    return _run_bank(x, h, mode, block, out, fft, False)


def correlate_bank(x, h, mode: str = "full", block: Optional[int] = None, out: str = "real", fft: Optional[HipFftImpl] = None) -> np.ndarray:
    """numpy.correlate(x[r], h[f], mode) for every row r and every filter f (the taps reversed, complex ones conjugated), in f32 by
    overlap-save.  The modes are the windows of the full result: "same" starts at (nh - 1) // 2."""
    return _run_bank(x, h, mode, block, out, fft, True)
