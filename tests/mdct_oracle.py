"""Expected values of the fast DCT-IV, the MDCT and the IMDCT of rows: the definition of include/kofft_hip.h in numpy
float32 over the CPU oracle's fft (its threaded entry; a length that is not a power of two takes its Bluestein arm).  Complex::mul
(num.rs:162-165) is done on the .real and .imag views as four f32 products, one subtract and one add (numpy's complex64 multiply may
fuse or reorder).  The twiddle tables are the library's own host function, kofft_hip_dct4_table_f32, which needs no device."""
from __future__ import annotations

import ctypes as C

import numpy as np

F = np.float32


def tables(n: int):
    """(c, d): the two complex64 tables of n / 2 entries each."""
    from kofft_amd import _lib

    out = np.empty(2 * n, F)
    rc = _lib.load().kofft_hip_dct4_table_f32(n, C.c_void_p(out.ctypes.data))
    assert rc == 0, rc
    t = out.view(np.complex64)
    return t[:n // 2].copy(), t[n // 2:].copy()


def _cmul(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    out = np.empty(np.broadcast(a, b).shape, np.complex64)
    with np.errstate(invalid="ignore", over="ignore"):  # (special-value tests: Inf * 0 and Inf - Inf are the expected NaNs)
        out.real = a.real * b.real - a.imag * b.imag
        out.imag = a.real * b.imag + a.imag * b.real
    return out


def dct4_ref(u: np.ndarray) -> np.ndarray:
    """dct4_fast of every row of the [rows, N] float32 array u, N even."""
    from oracle import pyoracle

    u = np.ascontiguousarray(u, F)
    assert u.ndim == 2 and u.shape[1] % 2 == 0 and u.shape[1] > 0
    rows, n = u.shape
    m = n // 2
    c, d = tables(n)
    z = np.empty((rows, m), np.complex64)
    z.real = u[:, 0::2]
    z.imag = u[:, ::-1][:, 0::2]  # u[N-1-2j]
    z = _cmul(z, c[None, :])
    Z = pyoracle.fft_mt(z) if m > 1 and rows else z
    y = _cmul(Z, d[None, :])
    out = np.empty((rows, n), F)
    out[:, 0::2] = y.real
    out[:, ::-1][:, 0::2] = -y.imag  # X[N-1-2k]
    return out


def windowed_frames(x: np.ndarray, w: np.ndarray, lead: int, frames: int) -> np.ndarray:
    """[rows, frames, 2N] float32: g[i] = x[f N + i - lead] * w[i] where the sample exists, +0 elsewhere."""
    x = np.ascontiguousarray(x, F)
    w = np.ascontiguousarray(w, F)
    rows, nx = x.shape
    n = w.size // 2
    assert w.size == 2 * n and 0 <= lead < 2 * n
    g = np.zeros((rows, frames, 2 * n), F)
    for f in range(frames):
        s0 = f * n - lead
        lo, hi = max(0, -s0), min(2 * n, nx - s0)
        if lo < hi:
            with np.errstate(invalid="ignore", over="ignore"):
                g[:, f, lo:hi] = x[:, s0 + lo:s0 + hi] * w[None, lo:hi]
    return g


def fold(g: np.ndarray) -> np.ndarray:
    """[..., 2N] -> [..., N]: u[j] = (-g[3N/2-1-j]) - g[3N/2+j] for j < N/2, g[j-N/2] - g[3N/2-1-j] beyond."""
    n = g.shape[-1] // 2
    h, q = n // 2, n + n // 2
    u = np.empty(g.shape[:-1] + (n,), F)
    j, k = np.arange(h), np.arange(h, n)
    with np.errstate(invalid="ignore"):
        u[..., :h] = (-g[..., q - 1 - j]) - g[..., q + j]
        u[..., h:] = g[..., k - h] - g[..., q - 1 - k]
    return u


def unfold(v: np.ndarray) -> np.ndarray:
    """[..., N] -> [..., 2N]: y[i] = v[N/2+i] for i < N/2, -v[3N/2-1-i] for N/2 <= i < 3N/2, -v[i-3N/2] beyond."""
    n = v.shape[-1]
    h, q = n // 2, n + n // 2
    y = np.empty(v.shape[:-1] + (2 * n,), F)
    y[..., :h] = v[..., h:]
    y[..., h:q] = -v[..., ::-1]
    y[..., q:] = -v[..., :h]
    return y


def mdct_ref(x: np.ndarray, w: np.ndarray, lead: int, frames: int) -> np.ndarray:
    """[rows, frames, N] float32 coefficients of the [rows, nx] float32 array x."""
    g = windowed_frames(x, w, lead, frames)
    rows, _, n2 = g.shape
    u = fold(g)
    return dct4_ref(u.reshape(rows * frames, n2 // 2)).reshape(rows, frames, n2 // 2)


def imdct_ref(X: np.ndarray, w: np.ndarray, scale) -> np.ndarray:
    """[rows, (frames + 1) N] float32: the whole overlap-added result of the [rows, frames, N] coefficients."""
    X = np.ascontiguousarray(X, F)
    w = np.ascontiguousarray(w, F)
    rows, frames, n = X.shape
    scale = F(scale)
    y = unfold(dct4_ref(X.reshape(rows * frames, n))).reshape(rows, frames, 2 * n)
    with np.errstate(invalid="ignore", over="ignore"):
        t = y * w[None, None, :]
        full = np.empty((rows, frames + 1, n), F)
        full[:, 0] = t[:, 0, :n] * scale
        full[:, frames] = t[:, frames - 1, n:] * scale
        if frames > 1:
            full[:, 1:frames] = (t[:, :-1, n:] + t[:, 1:, :n]) * scale
    return full.reshape(rows, (frames + 1) * n)
