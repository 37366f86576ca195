"""Expected values of cepstrum::real_cepstrum (cepstrum.rs:12-33), composed from the CPU oracle (its threaded entries): the oracle's fft of (x, +0), the
magnitude sqrt(re * re + im * im) on the .real and .imag views in float32 (one rounding per operation: not hypot), the libm crate's
logf of mag + 1e-12f (restated below, vectorised), then (l, +0) through the oracle's ifft (conj, fft, conj * 1/n; n == 1 returns
early) and its real parts.  Written apart from the device's restatement (kofft_amd/csrc/libm_logf.hip.h): the two agreeing bit for bit
on the device is the second opinion."""
from __future__ import annotations

import numpy as np

# libm 0.2 logf.rs (the musl / FreeBSD e_logf.c port), constants by their bits
_U = np.uint32
LN2_HI = np.array(0x3F317180, _U).view(np.float32)[()]
LN2_LO = np.array(0x3717F7D1, _U).view(np.float32)[()]
LG1 = np.array(0x3F2AAAAA, _U).view(np.float32)[()]
LG2 = np.array(0x3ECCCE13, _U).view(np.float32)[()]
LG3 = np.array(0x3E91E9EE, _U).view(np.float32)[()]
LG4 = np.array(0x3E789E26, _U).view(np.float32)[()]
EPS = np.float32(1e-12)  # cepstrum.rs:28: 1e-12 as an f32 (bits 0x2b8cbccc)


def libm_logf(x) -> np.ndarray:
    """logf of libm 0.2 on a float32 array: every operation a float32 operation (numpy rounds each one), bits through view(uint32)."""
    x = np.array(x, np.float32, copy=True, ndmin=1)
    f32 = np.float32
    ix = x.view(_U).copy()
    k = np.zeros(x.shape, np.int32)
    out = np.zeros(x.shape, np.float32)
    done = np.zeros(x.shape, bool)
    with np.errstate(all="ignore"):
        small_or_neg = (ix < _U(0x00800000)) | ((ix >> _U(31)) != 0)
        zero = small_or_neg & ((ix << _U(1)) == 0)
        out[zero] = f32(-1.0) / (x[zero] * x[zero])  # log(+-0) = -inf
        done |= zero
        neg = small_or_neg & ~done & ((ix >> _U(31)) != 0)
        out[neg] = (x[neg] - x[neg]) / f32(0.0)  # log(-x) = NaN
        done |= neg
        sub = small_or_neg & ~done
        k[sub] -= 25
        x[sub] = x[sub] * np.array(0x4C000000, _U).view(np.float32)[()]  # 2^25
        ix[sub] = x[sub].view(_U)
        big = ~small_or_neg & (ix >= _U(0x7F800000))
        out[big] = x[big]  # +inf, NaN
        done |= big
        one = ~small_or_neg & ~done & (ix == _U(0x3F800000))
        out[one] = f32(0.0)
        done |= one
        m = ~done
        ixm = ix[m] + _U(0x3F800000 - 0x3F3504F3)
        km = k[m] + (ixm >> _U(23)).astype(np.int32) - 0x7F
        ixm = (ixm & _U(0x007FFFFF)) + _U(0x3F3504F3)
        xm = ixm.view(np.float32)
        f = xm - f32(1.0)
        s = f / (f32(2.0) + f)
        z = s * s
        w = z * z
        t1 = w * (LG2 + w * LG4)
        t2 = z * (LG1 + w * LG3)
        r = t2 + t1
        hfsq = f32(0.5) * f * f
        dk = km.astype(np.float32)
        out[m] = s * (hfsq + r) + dk * LN2_LO - hfsq + f + dk * LN2_HI
    return out


def cepstrum_ref(rows: np.ndarray) -> np.ndarray:
    """The real cepstrum of every row of a [batch, n] float32 array (n a power of two), as the reference computes it."""
    from oracle import pyoracle

    x = np.ascontiguousarray(rows, np.float32)
    assert x.ndim == 2 and x.shape[1] > 0 and x.shape[1] & (x.shape[1] - 1) == 0
    freq = np.zeros(x.shape, np.complex64)  # Complex32::new(x, 0.0): imaginary parts +0
    freq.real = x
    spec = pyoracle.fft_mt(freq)
    re, im = spec.real.copy(), spec.imag.copy()
    with np.errstate(all="ignore"):
        mag = np.sqrt(re * re + im * im)  # float32 throughout: two multiplies, one add, a correctly rounded root
        l = libm_logf((mag + EPS).reshape(-1)).reshape(x.shape)
    logspec = np.zeros(x.shape, np.complex64)  # c.im = 0.0
    logspec.real = l
    return np.ascontiguousarray(pyoracle.fft_mt(logspec, inverse=True).real)
