"""Expected values of DctPlanner::plan_dct2 (dct.rs:61-105), composed from the CPU oracle: the oracle's rfft (threaded entry) of the mirrored
2n-sample rows (dct.rs:77-86), then the f32 twist of dct.rs:87-92 in numpy (float32 arrays: one rounding per operation,
nothing fused).  The angle's cosine and sine come from glibc's cosf / sinf, which Rust's f32::cos / f32::sin call on
linux-gnu; this module is test infrastructure, not the library's table (tables.cpp), which tests/test_dct_tables.py checks
against it."""
from __future__ import annotations

import ctypes as C

import numpy as np

_libm = C.CDLL("libm.so.6")
_libm.cosf.restype = C.c_float
_libm.cosf.argtypes = [C.c_float]
_libm.sinf.restype = C.c_float
_libm.sinf.argtypes = [C.c_float]

_cache: dict[int, tuple[np.ndarray, np.ndarray]] = {}


def angles(n: int) -> np.ndarray:
    """PI * (k as f32) / (2.0 * (n as f32)) for k < n, every step in f32 (dct.rs:54, 90)."""
    k = np.arange(n, dtype=np.int64).astype(np.float32)
    return (np.float32(np.pi) * k) / (np.float32(2.0) * np.float32(n))


def cos_sin(n: int) -> tuple[np.ndarray, np.ndarray]:
    """glibc cosf / sinf of angles(n), one call per value."""
    if n not in _cache:
        a = angles(n)
        c = np.fromiter((_libm.cosf(float(v)) for v in a), np.float32, n)
        s = np.fromiter((_libm.sinf(float(v)) for v in a), np.float32, n)
        _cache[n] = (c, s)
    return _cache[n]


def dct2_ref(rows: np.ndarray) -> np.ndarray:
    """DCT-II of every row of a [batch, n] float32 array, as the reference computes it."""
    from oracle import pyoracle

    x = np.ascontiguousarray(rows, np.float32)
    assert x.ndim == 2 and x.shape[1] > 0
    n = x.shape[1]
    buf = np.concatenate([x, x[:, ::-1]], axis=1)  # buf[i] = buf[2n-1-i] = x[i]
    spec = pyoracle.rfft_mt(buf)[:, :n]
    c, s = cos_sin(n)
    return np.float32(0.5) * (spec.real * c + spec.imag * s)


def dct2_f64(rows: np.ndarray) -> np.ndarray:
    """The textbook unnormalised DCT-II, sum_i x[i] cos(PI k (2i + 1) / (2n)), as a float64 matrix product."""
    x = np.asarray(rows, np.float64)
    n = x.shape[1]
    k = np.arange(n)[:, None]
    i = np.arange(n)[None, :]
    return x @ np.cos(np.pi * k * (2 * i + 1) / (2 * n)).T
