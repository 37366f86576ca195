"""Expected values of cepstrum::mel_filterbank / mfcc (cepstrum.rs:36-85) with the filter edges as an input, restated from the
reference's loops alone in numpy float32: the two loops of every filter, sequential in k and vectorised over rows only (one division,
one multiply, one add per term, each rounded to f32); cepstrum_oracle.libm_logf of e + 1e-12f; trig_direct_oracle's dct::dct2, first
num_coeffs outputs.  ref_bins is the f32 formula of cepstrum.rs:38-50 with the C library's log10f / powf through ctypes, bins_f64 the
floor of the same formula in float64.  Test infrastructure: nothing here calls the library."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

import cepstrum_oracle as co
import trig_direct_oracle as tdo

_libm = C.CDLL("libm.so.6")
for _f, _n in (("log10f", 1), ("powf", 2), ("floorf", 1)):
    getattr(_libm, _f).restype = C.c_float
    getattr(_libm, _f).argtypes = [C.c_float] * _n

F = np.float32
U64_MAX = (1 << 64) - 1

# (sample rate, n_fft, filters): every exact edge at least 1.5e-3 from an integer, so the f32 floor is the float64 floor
SETTINGS = [(16000, 32, 8), (16000, 256, 26), (16000, 512, 40), (48000, 512, 40), (22050, 1024, 128), (8000, 8, 40), (16000, 64, 13)]


def _sat(v: float) -> int:
    """Rust's `as usize` of an f32: NaN and negatives 0, saturating at the top."""
    if not v > 0:
        return 0
    return U64_MAX if v >= 2.0 ** 64 else int(v)


def ref_bins(sample_rate, n_fft: int, num_filters: int) -> list[int]:
    """cepstrum.rs:38-50 in f32, Rust's parse order."""
    with np.errstate(all="ignore"):
        sr = F(sample_rate)
        f_max = sr / F(2.0)
        mel_min = F(2595.0) * F(_libm.log10f(F(1.0) + F(0.0) / F(700.0)))
        mel_max = F(2595.0) * F(_libm.log10f(F(1.0) + f_max / F(700.0)))
        out = []
        for i in range(num_filters + 2):
            p = mel_min + (mel_max - mel_min) * F(i) / F(num_filters + 1)
            p = F(700.0) * (F(_libm.powf(F(10.0), p / F(2595.0))) - F(1.0))
            out.append(_sat(float(_libm.floorf(p * (F(n_fft) + F(1.0)) / sr))))
    return out


def edges_f64(sample_rate, n_fft: int, num_filters: int) -> list[float]:
    """The same formula in float64, before the floor."""
    mel_max = 2595.0 * math.log10(1.0 + (sample_rate / 2.0) / 700.0)
    out = []
    for i in range(num_filters + 2):
        p = mel_max * i / (num_filters + 1)
        out.append(700.0 * (10.0 ** (p / 2595.0) - 1.0) * (n_fft + 1.0) / sample_rate)
    return out


def _f(v: int) -> np.float32:
    """`v as f32` of a usize: rounded to nearest."""
    return np.array(v, np.uint64).astype(F)[()]


def energies(x: np.ndarray, bins) -> np.ndarray:
    """cepstrum.rs:51-67 on every row of a [rows, n_fft] float32 array: [rows, num_mel]."""
    x = np.ascontiguousarray(x, F)
    rows, n = x.shape
    bins = [int(b) for b in bins]
    num_mel = len(bins) - 2
    out = np.zeros((rows, max(num_mel, 0)), F)
    with np.errstate(all="ignore"):
        for m in range(1, num_mel + 1):
            a, b, c = bins[m - 1], bins[m], bins[m + 1]
            if b == a or c == b:
                continue
            acc = np.zeros(rows, F)
            for k in range(a, min(b, n)):  # fft_mags.get(k): terms past the row are skipped
                acc = acc + (_f(k - a) / _f(b - a)) * x[:, k]
            for k in range(b, min(c, n)):
                acc = acc + (_f(c - k) / _f(c - b)) * x[:, k]
            out[:, m - 1] = acc
    return out


def log_mel(e: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        return co.libm_logf((e + co.EPS).reshape(-1)).reshape(e.shape)


def mfcc(x: np.ndarray, bins, num_coeffs: int) -> np.ndarray:
    """cepstrum.rs:78-84: [rows, num_coeffs]."""
    lm = log_mel(energies(x, bins))
    return np.ascontiguousarray(tdo.direct("dct", 2, lm)[:, :num_coeffs])


def live(bins) -> list[bool]:
    bins = [int(b) for b in bins]
    return [bins[m + 1] != bins[m] and bins[m + 2] != bins[m + 1] for m in range(len(bins) - 2)]
