"""NumPy restatement of the Hermitian completion the one-sided ISTFT applies to its input (include/kofft_hip.h, "one-sided STFT"): the
reference of the GPU tests.  Test infrastructure only."""
from __future__ import annotations

import numpy as np


# the round-trip cases of tests/test_gpu_stft_onesided.py: (win_len, hop, seed); len = 9 * hop + 17
ROUND_TRIPS = [(256, 64, 67256), (1024, 256, 68024), (400, 160, 67400)]


def round_trip_signal(win_len: int, hop: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).uniform(-1, 1, 9 * hop + 17).astype(np.float32)


def bins(n: int) -> int:
    return n // 2 + 1


def complete(half: np.ndarray, n: int) -> np.ndarray:
    """[..., n // 2 + 1] complex64 -> [..., n]: F[k] = H[k] for k <= n / 2, (H[n - k].re, -H[n - k].im) above.  The imaginary parts of
    H[0] and H[n / 2] are used as given; the negation flips the sign bit and nothing else (so -(+0) is -0)."""
    half = np.ascontiguousarray(half, np.complex64)
    k_bins = bins(n)
    if half.shape[-1] != k_bins:
        raise ValueError(f"last axis {half.shape[-1]}, want {k_bins}")
    full = np.empty(half.shape[:-1] + (n,), np.complex64)
    full[..., :k_bins] = half
    for k in range(k_bins, n):
        src = half[..., n - k]
        full[..., k].real = src.real
        full[..., k].imag = np.negative(src.imag)
    return full


def round_trip_errors(oracle, x: np.ndarray, win: np.ndarray, hop: int):
    """With the oracle alone: (error of the one-sided round trip, error of the full round trip) of one signal, each the largest
    absolute error over the samples at least win.size from either end.  The one-sided trip keeps bins 0 .. n/2 of oracle.stft,
    completes them and hands them to oracle.istft."""
    n, length = win.size, x.size
    frames = -(-length // hop)
    spec = oracle.stft(x, win, hop, frames)
    full = oracle.istft(spec.copy(), win, hop, length)
    one = oracle.istft(complete(spec[:, :bins(n)], n), win, hop, length)
    mid = slice(n, length - n)
    return float(np.abs(one[mid] - x[mid]).max()), float(np.abs(full[mid] - x[mid]).max())
