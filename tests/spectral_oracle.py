"""Expected values of czt::czt_f32 (czt.rs:16-54) and goertzel::goertzel_f32 (goertzel.rs:16-36, the std form), restated from the
reference's loops alone in numpy float32: every operation one f32 rounding in the reference's order, nothing fused.  The vectorised
forms run over (row, k) or (row, frequency) and loop over the samples; the *_scalar forms are line-by-line transcriptions of the Rust
loops that tests/test_spectral_cpu.py holds the vectorised forms against on small cases.  glibc's cosf (Rust's f32::cos on linux-gnu)
and floorf come through ctypes.  This module is test infrastructure and does not use the library."""
from __future__ import annotations

import ctypes as C

import numpy as np

_libm = C.CDLL("libm.so.6")
for _f in ("cosf", "floorf"):
    getattr(_libm, _f).restype = C.c_float
    getattr(_libm, _f).argtypes = [C.c_float]

_F = np.float32
_PI = _F(np.pi)  # core::f32::consts::PI
_QUIET = dict(over="ignore", invalid="ignore", under="ignore", divide="ignore")


def _pair(z):
    """A complex number or (re, im) as two np.float32."""
    if isinstance(z, (tuple, list, np.ndarray)):
        return _F(z[0]), _F(z[1])
    z = complex(z)
    return _F(z.real), _F(z.imag)


def _mul(pr, pi, qr, qi):
    """czt.rs:28-29: (p.r * q.r - p.i * q.i, p.r * q.i + p.i * q.r), each product and each sum rounded to f32."""
    return pr * qr - pi * qi, pr * qi + pi * qr


def a_inv(a):
    """czt.rs:19-21."""
    ar, ai = _pair(a)
    with np.errstate(**_QUIET):
        denom = ar * ar + ai * ai
        if denom == 0:
            return _F(0), _F(0)
        return ar / denom, -ai / denom


def czt_wpow(m: int, w) -> np.ndarray:
    """[m, 2]: w multiplied k times into (1, 0) (czt.rs:25-32 restarts at every k; the running prefix takes the same steps)."""
    wr, wi = _pair(w)
    out = np.empty((m, 2), _F)
    pr, pi = _F(1), _F(0)
    with np.errstate(**_QUIET):
        for k in range(m):
            out[k] = pr, pi
            pr, pi = _mul(pr, pi, wr, wi)
    return out


def czt_apow(n: int, a) -> np.ndarray:
    """[n, 2]: a_inv multiplied i times into (1, 0) (czt.rs:35-36, 47-50)."""
    ir, ii = a_inv(a)
    out = np.empty((n, 2), _F)
    pr, pi = _F(1), _F(0)
    with np.errstate(**_QUIET):
        for i in range(n):
            out[i] = pr, pi
            pr, pi = _mul(pr, pi, ir, ii)
    return out


def _walk(n: int, m: int, w, a):
    """Yields (i, tr[m], ti[m]): the term factors of sample i for every bin (czt.rs:38-39), wnk advanced as czt.rs:43-46."""
    wp, ap = czt_wpow(m, w), czt_apow(n, a)
    wkr, wki = wp[:, 0].copy(), wp[:, 1].copy()
    wr, wi = np.ones(m, _F), np.zeros(m, _F)
    with np.errstate(**_QUIET):
        for i in range(n):
            tr, ti = _mul(ap[i, 0], ap[i, 1], wr, wi)
            yield i, tr, ti
            wr, wi = _mul(wr, wi, wkr, wki)


def czt_table(n: int, m: int, w, a) -> np.ndarray:
    """[n, 2 m] float32: C[i][2k], C[i][2k + 1] = apow[i] * wnk_k[i]."""
    c = np.zeros((n, 2 * m), _F)
    for i, tr, ti in _walk(n, m, w, a):
        c[i, 0::2] = tr
        c[i, 1::2] = ti
    return c


def czt(x, m: int, w, a) -> np.ndarray:
    """[batch, m] complex64 for a [batch, n] float32 input (a 1-D input: [m])."""
    x = np.asarray(x, _F)
    rows = x.reshape(1, -1) if x.ndim == 1 else x
    batch, n = rows.shape
    outr, outi = np.zeros((batch, m), _F), np.zeros((batch, m), _F)
    with np.errstate(**_QUIET):
        for i, tr, ti in _walk(n, m, w, a):
            xi = rows[:, i:i + 1]
            outr = outr + xi * tr[None, :]  # czt.rs:40-41
            outi = outi + xi * ti[None, :]
    out = np.empty((batch, m), np.complex64)
    out.real, out.imag = outr, outi
    return out[0] if x.ndim == 1 else out


def czt_scalar(x, m: int, w, a) -> np.ndarray:
    """czt.rs:16-54 line by line on one row, np.float32 scalars throughout."""
    wr, wi = _pair(w)
    a_inv_r, a_inv_i = a_inv(a)
    out = np.zeros(m, np.complex64)
    with np.errstate(**_QUIET):
        for k in range(m):
            w_k_r, w_k_i = _F(1), _F(0)
            for _ in range(k):
                tr = w_k_r * wr - w_k_i * wi
                ti = w_k_r * wi + w_k_i * wr
                w_k_r, w_k_i = tr, ti
            wnk_r, wnk_i, a_pow_r, a_pow_i = _F(1), _F(0), _F(1), _F(0)
            o0, o1 = _F(0), _F(0)
            for xv in np.asarray(x, _F):
                tr = a_pow_r * wnk_r - a_pow_i * wnk_i
                ti = a_pow_r * wnk_i + a_pow_i * wnk_r
                o0 = o0 + xv * tr
                o1 = o1 + xv * ti
                wtr = wnk_r * w_k_r - wnk_i * w_k_i
                wti = wnk_r * w_k_i + wnk_i * w_k_r
                wnk_r, wnk_i = wtr, wti
                atr = a_pow_r * a_inv_r - a_pow_i * a_inv_i
                ati = a_pow_r * a_inv_i + a_pow_i * a_inv_r
                a_pow_r, a_pow_i = atr, ati
            out.real[k], out.imag[k] = o0, o1
    return out


def goertzel_coeff(n: int, sample_rate, freqs) -> np.ndarray:
    """goertzel.rs:23-26 per frequency: [nfreq] float32."""
    nf = _F(n)
    rate = _F(sample_rate)
    out = np.empty(len(freqs), _F)
    with np.errstate(**_QUIET):
        for j, f in enumerate(np.asarray(freqs, _F)):
            k = _F(_libm.floorf(C.c_float(float((f * nf) / rate))))
            omega = ((_F(2) * _PI) * k) / nf
            out[j] = _F(2) * _F(_libm.cosf(C.c_float(float(omega))))
    return out


def goertzel(x, sample_rate, freqs) -> np.ndarray:
    """[batch, nfreq] float32 for a [batch, n] float32 input, n >= 1 (the argument errors are the caller's)."""
    x = np.asarray(x, _F)
    rows = x.reshape(1, -1) if x.ndim == 1 else x
    batch, n = rows.shape
    c = goertzel_coeff(n, sample_rate, freqs)[None, :]
    s1 = np.zeros((batch, c.shape[1]), _F)
    s2 = np.zeros_like(s1)
    with np.errstate(**_QUIET):
        for i in range(n):
            s = (rows[:, i:i + 1] + c * s1) - s2  # goertzel.rs:30
            s2, s1 = s1, s
        power = (s2 * s2 + s1 * s1) - (c * s1) * s2  # goertzel.rs:34
        out = np.sqrt(power)
    return out[0] if x.ndim == 1 else out


def goertzel_scalar(x, sample_rate, target_freq) -> np.float32:
    """goertzel.rs:16-36 line by line on one row and one frequency (after its two error returns)."""
    coeff = goertzel_coeff(len(x), sample_rate, [target_freq])[0]
    s_prev, s_prev2 = _F(0), _F(0)
    with np.errstate(**_QUIET):
        for xv in np.asarray(x, _F):
            s = xv + coeff * s_prev - s_prev2
            s_prev2 = s_prev
            s_prev = s
        power = s_prev2 * s_prev2 + s_prev * s_prev - coeff * s_prev * s_prev2
        return np.sqrt(power)


# The parameter sets of the device tests: name -> (w, a) for m bins
def param_sets(m: int) -> dict:
    two_pi = 2.0 * np.pi
    return {
        "dft": (np.exp(-1j * two_pi / max(m, 1)), 1.0 + 0j),
        "zoom": (np.exp(-1j * two_pi * 0.001), np.exp(1j * two_pi * 0.1)),
        "spiral": (0.99 * np.exp(-1j * 0.3), 1.01 * np.exp(1j * 0.2)),
        "a_zero": (np.exp(-1j * two_pi * 0.01), 0j),
        "grow": (1.5 * np.exp(-1j * 0.1), 1.0 + 0j),
    }
