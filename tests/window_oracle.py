"""Test oracle of the windows beyond Hann (window.rs:31-61, window_more.rs:13-64), written apart from kofft_amd/csrc/tables.cpp:
every expression in float32 in Rust's parse order, `.cos()` through glibc's cosf (ctypes), the libm crate's cosf / sinf through
hartley_oracle's numpy restatement, sqrtf as numpy's correctly rounded float32 root."""
import ctypes as C

import numpy as np

from hartley_oracle import cosf as crate_cosf, sinf as crate_sinf

F = np.float32
PI = F(np.pi)  # core::f32::consts::PI
_libm = C.CDLL("libm.so.6")
_libm.cosf.restype = C.c_float
_libm.cosf.argtypes = [C.c_float]

KINDS = ("hamming", "blackman", "kaiser", "tukey", "bartlett", "bohman", "nuttall")  # KOFFT_WINDOW_* 0 .. 6


def glibc_cosf(a):
    a = np.asarray(a, F)
    return np.fromiter((_libm.cosf(float(v)) for v in a.ravel()), F, a.size).reshape(a.shape)


def _idx(length):
    return np.arange(length, dtype=np.int64).astype(F)  # `i as f32`


def hamming(length):
    return F(0.54) - F(0.46) * glibc_cosf(F(2.0) * PI * _idx(length) / F(length))


def blackman(length):
    x = _idx(length) / F(length)
    return F(0.42) - F(0.5) * glibc_cosf(F(2.0) * PI * x) + F(0.08) * glibc_cosf(F(4.0) * PI * x)


def bessel0(x):
    """window.rs:9-21, on a float32 array."""
    x = np.asarray(x, F)
    total = np.ones(x.shape, F)
    y = x * x / F(4.0)
    t = y.copy()
    k = F(1.0)
    for n in range(1, 20):
        k = k * F(n)
        total = total + t / (k * k)
        t = t * y
    return total


def kaiser(length, beta):
    if length == 0:
        raise ValueError("kaiser(0, beta): the reference underflows len - 1")
    beta = F(beta)
    denom = bessel0(beta)
    m = F(length - 1) / F(2.0)
    r = (_idx(length) - m) / m
    return bessel0(beta * np.sqrt(F(1.0) - r * r)) / denom


def _as_usize(v):
    """Rust's saturating `as usize` of an f32."""
    if not v > 0:  # NaN, negatives, zeros
        return 0
    return min(int(v), 2 ** 64 - 1) if np.isfinite(v) else 2 ** 64 - 1


def tukey(length, alpha):
    alpha = F(alpha)
    if alpha < F(0.0):  # f32::clamp(0.0, 1.0): a NaN passes both comparisons and stays
        alpha = F(0.0)
    if alpha > F(1.0):
        alpha = F(1.0)
    lenf = F(length)
    edge = _as_usize(np.floor(alpha * (lenf - F(1.0)) / F(2.0)))
    w = np.zeros(length, F)
    for n in range(length):
        nf = F(n)
        if n < edge:
            w[n] = F(0.5) * (F(1.0) + glibc_cosf(PI * (F(2.0) * nf / (alpha * (lenf - F(1.0))) - F(1.0))))
        elif n < length - edge:
            w[n] = F(1.0)
        else:
            w[n] = F(0.5) * (F(1.0) + glibc_cosf(PI * (F(2.0) * nf / (alpha * (lenf - F(1.0))) - F(2.0) / alpha + F(1.0))))
    return w


def bartlett(length):
    n = F(length)
    x = (_idx(length) - (n - F(1.0)) / F(2.0)) / ((n - F(1.0)) / F(2.0))
    return F(1.0) - np.abs(x)


def bohman(length):
    x = (_idx(length) / (F(length) - F(1.0))) - F(0.5)
    return (F(1.0) - np.abs(x)) * crate_cosf(PI * x) + F(1.0) / PI * crate_sinf(PI * x)


def nuttall(length):
    x = F(2.0) * PI * _idx(length) / (F(length) - F(1.0))
    return F(0.355768) - F(0.487396) * crate_cosf(x) + F(0.144232) * crate_cosf(F(2.0) * x) - F(0.012604) * crate_cosf(F(3.0) * x)


def window(kind, length, param=0.0):
    with np.errstate(all="ignore"):
        if kind == "kaiser":
            out = kaiser(length, param)
        elif kind == "tukey":
            out = tukey(length, param)
        else:
            out = {"hamming": hamming, "blackman": blackman, "bartlett": bartlett, "bohman": bohman, "nuttall": nuttall}[kind](length)
    out = np.asarray(out)
    assert out.dtype == F and out.shape == (length,), (kind, out.dtype, out.shape)
    return out
