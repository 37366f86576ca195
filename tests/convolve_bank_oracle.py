"""Expected values of the filter-bank overlap-save convolution / correlation of rows, composed from the CPU oracle (its
threaded entries) in the style of tests/convolve_oracle.py: the oracle's fft of the zero-padded taps of every filter -- real taps as
(h, +0), complex taps as they are, correlate: reversed and conjugated -- and of every frame (x, +0), once; per filter Complex::mul
(num.rs:162-165) on the .real and .imag views as four f32 products, one subtract and one add, then the oracle's ifft (conj, fft, conj *
1/block); of each frame's last hop points the real part, the complex value or the magnitude sqrt(re * re + im * im) in f32 (numpy's
float32 multiply, add and sqrt: un-fused, the root correctly rounded)."""
from __future__ import annotations

import numpy as np

KINDS = ("real", "complex", "magnitude")


def convolve_bank_ref(x: np.ndarray, h: np.ndarray, block: int, correlate: bool = False, out: str = "real") -> np.ndarray:
    """[rows, filters, nx + nh - 1]: every row of the [rows, nx] float32 array x convolved (correlate: cross-correlated) with every
    filter of the [filters, nh] float32 or complex64 bank h, by overlap-save with transforms of `block` points (a power of two >= nh).
    float32 for out = "real" / "magnitude", complex64 for "complex"."""
    from oracle import pyoracle

    assert out in KINDS
    x = np.ascontiguousarray(x, np.float32)
    h = np.asarray(h)
    taps = np.ascontiguousarray(h, np.complex64 if np.iscomplexobj(h) else np.float32)
    assert x.ndim == 2 and taps.ndim == 2
    rows, nx = x.shape
    filters, nh = taps.shape
    assert nx > 0 and nh > 0 and filters > 0
    assert block >= nh and block & (block - 1) == 0 and block >= 2
    hp = np.zeros((filters, block), np.complex64)  # real taps: (h[i], +0); then (+0, +0)
    if correlate:
        taps = taps[:, ::-1]
    if taps.dtype == np.complex64:
        hp.real[:, :nh] = taps.real
        hp.imag[:, :nh] = -taps.imag if correlate else taps.imag  # (the negation flips the sign of a zero as well, as conj does)
    else:
        hp.real[:, :nh] = taps
    H = pyoracle.fft_mt(hp)
    hop = block - nh + 1
    full = nx + nh - 1
    nb = -(-full // hop)
    # the row with nh - 1 zeros in front and enough behind: frame b is its samples [b * hop, b * hop + block)
    padded = np.zeros((rows, (nb - 1) * hop + block), np.float32)
    padded[:, nh - 1:nh - 1 + nx] = x
    frames = np.zeros((rows, nb, block), np.complex64)
    for b in range(nb):
        frames.real[:, b, :] = padded[:, b * hop:b * hop + block]
    X = pyoracle.fft_mt(frames.reshape(rows * nb, block)).reshape(rows, 1, nb, block)  # once for the whole bank
    Hb = H[None, :, None, :]
    Y = np.empty((rows, filters, nb, block), np.complex64)
    with np.errstate(invalid="ignore", over="ignore"):  # (special-value tests: Inf * 0 and Inf - Inf are the expected NaNs)
        Y.real = X.real * Hb.real - X.imag * Hb.imag
        Y.imag = X.real * Hb.imag + X.imag * Hb.real
    y = pyoracle.fft_mt(Y.reshape(rows * filters * nb, block), inverse=True).reshape(rows, filters, nb, block)
    kept = np.ascontiguousarray(y[:, :, :, nh - 1:]).reshape(rows, filters, nb * hop)[:, :, :full]
    if out == "real":
        return np.ascontiguousarray(kept.real)
    if out == "complex":
        return np.ascontiguousarray(kept)
    with np.errstate(invalid="ignore", over="ignore"):
        re, im = np.ascontiguousarray(kept.real), np.ascontiguousarray(kept.imag)
        return np.sqrt(re * re + im * im)
