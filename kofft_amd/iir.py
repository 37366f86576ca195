"""IIR filtering of f32 rows on the device by a cascade of second-order sections: scipy.signal.sosfilt's recurrence,
per row, section s (ascending) and sample t, with the section's input v and state (z0, z1)

    y = (b0 * v) + z0;   z0 = ((b1 * v) - (a1 * y)) + z1;   z1 = (b2 * v) - (a2 * y)

every product and sum one rounded float32 operation: bit for bit the definition in include/kofft_hip.h on every route, and bit for bit
scipy.signal.sosfilt on float32 arrays.  A row is filtered sequentially; the parallelism is across rows.

``sosfilt(sos, x, zi=None)`` is scipy.signal.sosfilt along the last axis: ``sos`` is [sections, 6] (b0 b1 b2 a0 a1 a2 with a0 == 1),
``x`` a 1-D signal or a 2-D [rows, nx] array, ``zi`` in scipy's layout ([sections, 2] or [sections, rows, 2]); with ``zi`` the result is
(y, zf).  ``reverse=True`` walks every row from its last sample to its first: flip(sosfilt(flip(x))) without the two copies.
``sosfilt_zi(sos)`` is scipy.signal.sosfilt_zi in closed form, float64, no device.  ``sosfiltfilt(sos, x)`` is the zero-phase
forward-backward filter **defined as this composition**: scipy's default ``padlen``, the odd extension in float32 (2 * x[0] - x[k]: one
product, one difference), a forward call with state float32(zi) * ext[0], a reverse call with state float32(zi) * y[last], the middle
nx samples.  Padding and the state products are numpy on the host; the two filter passes are the device calls.

``sosfilt_scan(sos, x, zi=None, chunk=None)`` is the same filter as a scan along time: every row is cut into chunks of
``chunk`` samples that are filtered in parallel, which is what makes a few long rows fast.  It has its own bit-exact definition
(include/kofft_hip.h): inside a chunk the recurrence above, at a seam the state M Z + p of the chunk's transition matrix, so its bits
differ from ``sosfilt``'s after the first chunk and depend on ``chunk``; it is as close to float64 scipy as ``sosfilt`` is.  ``chunk=None``
asks ``scan_chunk(rows, nx, sections)``, the measured choice (never below 1024).  Filtering a signal in two calls (zf -> zi) is correct but
not bit-identical to one call.  ``sosfiltfilt(..., chunk=...)`` runs its two passes through the scan.

``fft=`` names the f32 HipFftImpl to run on; without one, a context on device 0 is created at the first call and kept.  Shape and
value errors are raised before any context is created."""
from __future__ import annotations

from typing import Optional

import numpy as np

import ctypes as C

from . import _lib, api
from .api import FftError, HipFftImpl

__all__ = ["sosfilt", "sosfilt_scan", "scan_chunk", "sosfilt_zi", "sosfiltfilt", "default_padlen", "route"]

_default: Optional[HipFftImpl] = None


def route(rows: int) -> int:
    """kofft_hip_sosfilt_route: 1 where a default context runs the tiled kernel on a batch of ``rows`` rows, 0 where the plain one.  No
    device."""
    if int(rows) < 0:
        raise ValueError("rows is a usize: it cannot be negative")
    r = C.c_int()
    rc = _lib.load().kofft_hip_sosfilt_route(int(rows), C.byref(r))
    if rc:
        raise api.DeviceError(rc, "kofft_hip_sosfilt_route")
    return int(r.value)


def scan_chunk(rows: int, nx: int, sections: int) -> int:
    """kofft_hip_sosfilt_scan_chunk: the measured chunk for ``rows`` rows of ``nx`` samples through ``sections`` sections.  No device."""
    if min(int(rows), int(nx), int(sections)) < 0:
        raise ValueError("sizes are usize: they cannot be negative")
    r = C.c_size_t()
    rc = _lib.load().kofft_hip_sosfilt_scan_chunk(int(rows), int(nx), int(sections), C.byref(r))
    if rc:
        raise api.DeviceError(rc, "kofft_hip_sosfilt_scan_chunk")
    return int(r.value)


def _chunk(chunk, rows: int, nx: int, sections: int) -> int:
    if chunk is None:
        return scan_chunk(rows, nx, sections)
    k = int(chunk)
    if k <= 0 or k % 32:
        raise FftError(FftError.InvalidValue)  # (a multiple of KOFFT_HIP_SOSFILT_TILE)
    return k


def _sos(sos) -> np.ndarray:
    c = np.ascontiguousarray(sos, np.float32)
    if c.ndim != 2 or c.shape[1] != 6:
        raise TypeError("sos must be a [sections, 6] array")
    if c.shape[0] == 0:
        raise FftError(FftError.EmptyInput)
    if not (c[:, 3] == np.float32(1.0)).all():
        raise FftError(FftError.InvalidValue)  # (a0 is not divided by)
    return c


def _rows(x) -> np.ndarray:
    a = np.ascontiguousarray(x, np.float32)
    if a.ndim not in (1, 2):
        raise TypeError("expected a 1-D signal or a 2-D [rows, nx] array")
    return a


def _ctx(fft):
    global _default
    if fft is None:
        if _default is None:
            _default = api.HipFftImpl(np.float32)
        fft = _default
    return fft


def sosfilt(sos, x, zi=None, reverse: bool = False, fft: Optional[HipFftImpl] = None):
    """scipy.signal.sosfilt(sos, x, axis=-1, zi=zi) in float32: y, or (y, zf) when ``zi`` is given."""
    return _filter(sos, x, zi, reverse, fft, False, None)


def sosfilt_scan(sos, x, zi=None, chunk: Optional[int] = None, reverse: bool = False, fft: Optional[HipFftImpl] = None):
    """``sosfilt`` as a scan along time in chunks of ``chunk`` samples (a multiple of 32; None: ``scan_chunk``'s choice): the arguments,
    the state layout and the results of ``sosfilt``, the bits of kofft_hip_sosfilt_scan_f32's definition."""
    return _filter(sos, x, zi, reverse, fft, True, chunk)


def _filter(sos, x, zi, reverse, fft, scan: bool, chunk):
    c = _sos(sos)
    a = _rows(x)
    sections = c.shape[0]
    rows, nx = int(np.prod(a.shape[:-1], dtype=np.int64)), a.shape[-1]
    rows2d = a.reshape(rows, nx)
    if scan:
        chunk = _chunk(chunk, rows, nx, sections)
    st = None
    if zi is not None:
        z = np.asarray(zi, np.float32)
        if z.shape != (sections,) + a.shape[:-1] + (2,):
            raise FftError(FftError.MismatchedLengths)
        st = np.ascontiguousarray(z.reshape(sections, rows, 2).transpose(1, 0, 2))  # [rows, sections, 2], a copy
    if rows == 0 or nx == 0:
        y = np.empty(a.shape, np.float32)
        return y if zi is None else (y, np.array(zi, np.float32))
    fft = _ctx(fft)
    run = (lambda *p, **k: fft.sosfilt_scan_rows(*p, chunk, **k)) if scan else fft.sosfilt_rows
    if st is None:
        return run(rows2d, c, reverse=reverse).reshape(a.shape)
    y, zf = run(rows2d, c, zi=st, zf=True, reverse=reverse)
    return y.reshape(a.shape), np.ascontiguousarray(zf.transpose(1, 0, 2)).reshape((sections,) + a.shape[:-1] + (2,))


def sosfilt_zi(sos) -> np.ndarray:
    """scipy.signal.sosfilt_zi: the state of every section in the steady state of a unit step, [sections, 2] float64.  Per section
    K = (b0 + b1 + b2) / (1 + a1 + a2), z1 = b2 - a2 K, z0 = b1 - a1 K + z1, scaled by the product of the K of the sections before it."""
    c = np.asarray(sos, np.float64)
    if c.ndim != 2 or c.shape[1] != 6:
        raise TypeError("sos must be a [sections, 6] array")
    if not (c[:, 3] == 1.0).all():
        raise FftError(FftError.InvalidValue)
    zi = np.empty((c.shape[0], 2), np.float64)
    scale = 1.0
    for s, (b0, b1, b2, _, a1, a2) in enumerate(c):
        k = (b0 + b1 + b2) / (1.0 + a1 + a2)
        z1 = b2 - a2 * k
        z0 = b1 - a1 * k + z1
        zi[s] = scale * z0, scale * z1
        scale = scale * k
    return zi


def default_padlen(sos) -> int:
    """scipy.signal.sosfiltfilt's default: 3 * (2 * sections + 1 - min(#(b2 == 0), #(a2 == 0)))."""
    c = np.asarray(sos)
    return 3 * (2 * c.shape[0] + 1 - min(int((c[:, 2] == 0).sum()), int((c[:, 5] == 0).sum())))


def odd_ext(a: np.ndarray, n: int) -> np.ndarray:
    """scipy's odd extension of every float32 row by n samples on either side: 2 * x[0] - x[n .. 1], x, 2 * x[-1] - x[-2 .. -n - 1]."""
    if n == 0:
        return a
    two = np.float32(2.0)
    left = (two * a[:, :1]) - a[:, n:0:-1]
    right = (two * a[:, -1:]) - a[:, -2:-(n + 2):-1]
    return np.ascontiguousarray(np.concatenate([left, a, right], axis=1))


def sosfiltfilt(sos, x, padlen: Optional[int] = None, fft: Optional[HipFftImpl] = None, chunk: Optional[int] = None) -> np.ndarray:
    """The zero-phase forward-backward filter of every row (scipy.signal.sosfiltfilt with padtype "odd"), as the composition the
    module's docstring fixes.  ``chunk`` (a multiple of 32): both passes run through the scan in chunks of that many samples; without
    it, the sequential filter, as ever."""
    c = _sos(sos)
    a = _rows(x)
    if chunk is not None:
        chunk = _chunk(chunk, 0, 0, 0)
    edge = default_padlen(c) if padlen is None else int(padlen)
    if edge < 0:
        raise ValueError("padlen cannot be negative")
    nx = a.shape[-1]
    if nx <= edge:
        raise ValueError(f"the length of the input must be greater than padlen, which is {edge}")
    rows2d = a.reshape(int(np.prod(a.shape[:-1], dtype=np.int64)), nx)
    if rows2d.shape[0] == 0:
        return np.empty(a.shape, np.float32)
    zi = sosfilt_zi(c).astype(np.float32)  # [sections, 2]
    ext = odd_ext(rows2d, edge)
    fft = _ctx(fft)
    run = fft.sosfilt_rows if chunk is None else (lambda *p, **k: fft.sosfilt_scan_rows(*p, chunk, **k))
    y = run(ext, c, zi=np.ascontiguousarray(zi[None, :, :] * ext[:, :1, None]))
    y = run(y, c, zi=np.ascontiguousarray(zi[None, :, :] * y[:, -1:, None]), reverse=True)
    return np.ascontiguousarray(y[:, edge:edge + nx]).reshape(a.shape)
