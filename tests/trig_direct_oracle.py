"""Expected values of dct::dct1 .. dct4 (dct.rs:108-176) and dst::dst1 .. dst4 (dst.rs:89-146), restated from the reference's
loops alone: the angles in numpy float32 in the reference's order of operations, glibc's cosf / sinf through ctypes (Rust's
f32::cos / f32::sin on linux-gnu), and each output summed from its seed in increasing i with float32 numpy vector operations (one
multiply, then one add: nothing fused).  This module is test infrastructure and does not use the library's tables (tables.cpp);
tests/test_trig_direct_cpu.py checks those against it."""
from __future__ import annotations

import ctypes as C

import numpy as np

_libm = C.CDLL("libm.so.6")
for _f in ("cosf", "sinf"):
    getattr(_libm, _f).restype = C.c_float
    getattr(_libm, _f).argtypes = [C.c_float]

KINDS = [(fam, t) for fam in ("dct", "dst") for t in (1, 2, 3, 4)]
_F = np.float32
_PI = _F(np.pi)  # core::f32::consts::PI
_cache: dict = {}


def i_range(family: str, type: int, n: int) -> range:
    """The i of the reference's inner loop: dct1 take(n-1).skip(1); dct3 / dst3 skip(1); the rest every i."""
    if family == "dct" and type == 1:
        return range(1, max(n - 1, 1))
    if type == 3:
        return range(1, n)
    return range(0, n)


def angles(family: str, type: int, n: int, rows, cols) -> np.ndarray:
    """The f32 angle of term (i, k) for i in rows, k in cols: [len(rows), len(cols)]."""
    fi = np.asarray(rows, np.int64).astype(_F)[:, None]
    fk = np.asarray(cols, np.int64).astype(_F)[None, :]
    nf = _F(n)
    with np.errstate(all="ignore"):
        if family == "dct":
            if type == 1:
                return ((_PI / (nf - _F(1))) * fi) * fk
            f = _PI / nf
            if type == 2:
                return (f * (fi + _F(0.5))) * fk
            if type == 3:
                return (f * fi) * (fk + _F(0.5))
            return (f * (fi + _F(0.5))) * (fk + _F(0.5))
        if type == 1:
            return ((fi + _F(1)) * (fk + _F(1))) * (_PI / (nf + _F(1)))
        f = _PI / nf
        if type == 2:
            return (f * (fi + _F(0.5))) * (fk + _F(1))
        if type == 3:
            return (f * (fk + _F(0.5))) * fi
        return (f * (fi + _F(0.5))) * (fk + _F(0.5))


def table(family: str, type: int, n: int, rows=None, cols=None) -> np.ndarray:
    """C[i][k] for i in rows, k in cols (default: all n), glibc cosf / sinf per entry; rows outside the i range are +0."""
    rows = list(range(n)) if rows is None else [int(r) for r in rows]
    cols = list(range(n)) if cols is None else [int(c) for c in cols]
    key = (family, type, n, tuple(rows), tuple(cols))
    if key in _cache:
        return _cache[key]
    fn = _libm.cosf if family == "dct" else _libm.sinf
    rng = i_range(family, type, n)
    out = np.zeros((len(rows), len(cols)), _F)
    a = angles(family, type, n, rows, cols)
    for r, i in enumerate(rows):
        if i in rng:
            out[r] = np.fromiter((fn(float(v)) for v in a[r]), _F, len(cols))
    _cache[key] = out
    return out


def seed_and_x(family: str, type: int, x: np.ndarray, cols) -> tuple[np.ndarray, np.ndarray]:
    """(init [batch, len(cols)], x' [batch, n]) of the reference's loop."""
    b, n = x.shape
    k = np.asarray(cols, np.int64)[None, :]
    zero = np.zeros((b, len(cols)), _F)
    seed = lambda v: np.broadcast_to(v, (b, len(cols))).astype(_F)  # (not `zero + v`: +0 + -0 is +0)
    if family == "dct" and type == 1:
        if n == 1:
            with np.errstate(all="ignore"):
                return seed(x[:, :1] * _F(2.0)), x
        last = x[:, n - 1:n]
        with np.errstate(all="ignore"):
            init = np.where(k % 2 == 0, x[:, :1] + last, x[:, :1] + (-last)).astype(_F)
            return init, _F(2.0) * x
    if type == 3:
        return seed(x[:, :1] / _F(2.0)), x
    return zero, x  # `let mut sum = 0.0`: +0


def direct(family: str, type: int, x: np.ndarray, cols=None) -> np.ndarray:
    """The transform of every row of a [batch, n] float32 array at the outputs cols (default: all): [batch, len(cols)]."""
    x = np.ascontiguousarray(x, _F)
    b, n = x.shape
    if n == 0:
        return np.zeros((b, 0), _F)
    cols = list(range(n)) if cols is None else [int(c) for c in cols]
    c = table(family, type, n, None, cols)
    acc, xp = seed_and_x(family, type, x, cols)
    acc = acc.copy()
    with np.errstate(all="ignore"):
        for i in i_range(family, type, n):
            term = xp[:, i:i + 1] * c[i][None, :]  # one f32 multiply ...
            acc = acc + term                        # ... then one f32 add
    return acc


def sample_cols(n: int, count: int, seed: int) -> list[int]:
    """Seeded output columns for long rows, always with both ends and the tiled kernel's tile edges (multiples of 128 and their
    neighbours)."""
    fixed = {0, 1, n - 2, n - 1} | {e + d for e in range(128, n, 128) for d in (-1, 0)}
    rng = np.random.default_rng(seed)
    extra = set(rng.choice(n, size=min(count, n), replace=False).tolist())
    return sorted(c for c in fixed | extra if 0 <= c < n)


def matrix_f64(family: str, type: int, n: int) -> np.ndarray:
    """The textbook kernels of the eight transforms as float64 [n_i, n_k] matrices (DCT-I's end terms and the x0 / 2 seeds are left
    to direct_f64)."""
    i = np.arange(n, dtype=np.float64)[:, None]
    k = np.arange(n, dtype=np.float64)[None, :]
    if family == "dct":
        if type == 1:
            return 2.0 * np.cos(np.pi * i * k / max(n - 1, 1))
        if type == 2:
            return np.cos(np.pi / n * (i + 0.5) * k)
        if type == 3:
            return np.cos(np.pi / n * i * (k + 0.5))
        return np.cos(np.pi / n * (i + 0.5) * (k + 0.5))
    if type == 1:
        return np.sin(np.pi * (i + 1) * (k + 1) / (n + 1))
    if type == 2:
        return np.sin(np.pi / n * (i + 0.5) * (k + 1))
    if type == 3:
        return np.sin(np.pi / n * (k + 0.5) * i)
    return np.sin(np.pi / n * (i + 0.5) * (k + 0.5))


def direct_f64(family: str, type: int, x: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(value, sum of |terms|) of the transform in float64, from the textbook definitions."""
    x = np.asarray(x, np.float64)
    n = x.shape[1]
    m = matrix_f64(family, type, n)
    mask = np.zeros((n, 1))
    mask[list(i_range(family, type, n))] = 1.0
    m = m * mask
    val = x @ m
    mag = np.abs(x) @ np.abs(m)
    k = np.arange(n)[None, :]
    if family == "dct" and type == 1:
        if n == 1:
            return 2.0 * x[:, :1], 2.0 * np.abs(x[:, :1])
        ends = x[:, :1] + np.where(k % 2 == 0, 1.0, -1.0) * x[:, n - 1:n]
        val = val + ends
        mag = mag + np.abs(x[:, :1]) + np.abs(x[:, n - 1:n])
    elif type == 3:
        val = val + x[:, :1] / 2.0
        mag = mag + np.abs(x[:, :1]) / 2.0
    return val, mag
