"""Expected values of the overlap-save convolution / correlation of rows, composed from the CPU oracle (its threaded
entries): the oracle's fft of the zero-padded taps and of every frame (x, +0), Complex::mul (num.rs:162-165) on the .real and .imag
views as four f32 products, one subtract and one add (numpy's complex64 multiply may fuse or reorder), then the oracle's ifft (conj,
fft, conj * 1/block) and the real parts of each frame's last hop points."""
from __future__ import annotations

import numpy as np


def convolve_ref(x: np.ndarray, h: np.ndarray, block: int, correlate: bool = False) -> np.ndarray:
    """[rows, nx + nh - 1] float32: every row of the [rows, nx] float32 array x convolved (correlate: cross-correlated) with h, [nh]
    taps for all rows or [rows, nh] per row, by overlap-save with transforms of `block` points (a power of two >= nh)."""
    from oracle import pyoracle

    x = np.ascontiguousarray(x, np.float32)
    h = np.ascontiguousarray(h, np.float32)
    assert x.ndim == 2 and h.ndim in (1, 2)
    rows, nx = x.shape
    taps = h.reshape(-1, h.shape[-1])
    filters, nh = taps.shape
    assert filters in (1, rows) and nx > 0 and nh > 0
    assert block >= nh and block & (block - 1) == 0 and block >= 2
    if correlate:
        taps = taps[:, ::-1]
    hop = block - nh + 1
    full = nx + nh - 1
    nb = -(-full // hop)
    hp = np.zeros((filters, block), np.complex64)  # (h[i], +0), then (+0, +0)
    hp.real[:, :nh] = taps
    H = pyoracle.fft_mt(hp)
    # the row with nh - 1 zeros in front and enough behind: frame b is its samples [b * hop, b * hop + block)
    padded = np.zeros((rows, (nb - 1) * hop + block), np.float32)
    padded[:, nh - 1:nh - 1 + nx] = x
    frames = np.zeros((rows, nb, block), np.complex64)
    for b in range(nb):
        frames.real[:, b, :] = padded[:, b * hop:b * hop + block]
    X = pyoracle.fft_mt(frames.reshape(rows * nb, block)).reshape(rows, nb, block)
    Hb = H[:, None, :]  # one filter: broadcast over the rows
    Y = np.empty_like(X)
    with np.errstate(invalid="ignore", over="ignore"):  # (special-value tests: Inf * 0 and Inf - Inf are the expected NaNs)
        Y.real = X.real * Hb.real - X.imag * Hb.imag
        Y.imag = X.real * Hb.imag + X.imag * Hb.real
    y = pyoracle.fft_mt(Y.reshape(rows * nb, block), inverse=True).reshape(rows, nb, block)
    out = np.ascontiguousarray(y.real[:, :, nh - 1:]).reshape(rows, nb * hop)
    return np.ascontiguousarray(out[:, :full])
