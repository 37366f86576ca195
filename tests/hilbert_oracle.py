"""Expected values of hilbert::hilbert_analytic (hilbert.rs:13-47), composed from the CPU oracle (its threaded entries): the oracle's fft of (x, +0), the
mask of hilbert.rs:28-34 on the .real and .imag views separately (two f32 multiplies by 2 -- numpy's complex64 *= 2 is a complex
multiply, which turns an Inf into a NaN), then the oracle's ifft (conj, fft, conj * 1/n; n == 1 returns early)."""
from __future__ import annotations

import numpy as np


def hilbert_ref(rows: np.ndarray) -> np.ndarray:
    """The analytic signal of every row of a [batch, n] float32 array (n a power of two), as the reference computes it."""
    from oracle import pyoracle

    x = np.ascontiguousarray(rows, np.float32)
    assert x.ndim == 2 and x.shape[1] > 0 and x.shape[1] & (x.shape[1] - 1) == 0
    n = x.shape[1]
    freq = np.zeros(x.shape, np.complex64)  # Complex32::new(x, 0.0): imaginary parts +0
    freq.real = x
    spec = pyoracle.fft_mt(freq)
    if n % 2 == 0:
        h = n // 2
        spec.real[:, 1:h] *= np.float32(2.0)
        spec.imag[:, 1:h] *= np.float32(2.0)
        spec[:, h + 1:] = 0  # Complex32::zero(): (+0, +0)
    return pyoracle.fft_mt(spec, inverse=True)
