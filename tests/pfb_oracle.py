"""Expected values of the polyphase filter bank of rows, analysis and synthesis: the definitions of include/kofft_hip.h
in numpy float32 over the CPU oracle's fft (its threaded entry; a length that is not a power of two takes its Bluestein arm, and the
inverse is its conj, fft, conj, * 1 / M).  Products and sums are separate f32 operations on float32 arrays: numpy fuses nothing."""
from __future__ import annotations

import numpy as np

F = np.float32


def terms(x: np.ndarray, h: np.ndarray, hop: int, lead: int, frames: int) -> np.ndarray:
    """[rows, frames, nh] float32: h[i] * x[f D + i - lead] where the sample exists, +0 elsewhere."""
    x = np.ascontiguousarray(x, F)
    h = np.ascontiguousarray(h, F)
    rows, nx = x.shape
    nh = h.size
    assert 0 <= lead < nh and hop >= 1
    g = np.zeros((rows, frames, nh), F)
    for f in range(frames):
        s0 = f * hop - lead
        lo, hi = max(0, -s0), min(nh, nx - s0)
        if lo < hi:
            with np.errstate(invalid="ignore", over="ignore"):
                g[:, f, lo:hi] = h[None, lo:hi] * x[:, s0 + lo:s0 + hi]
    return g


def fold(g: np.ndarray, m: int) -> np.ndarray:
    """[..., T M] -> [..., M]: u[j] = (..((g[j] + g[j + M]) + g[j + 2M])..), one accumulator started by the first term."""
    taps = g.shape[-1] // m
    assert g.shape[-1] == taps * m
    u = g[..., :m].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(1, taps):
            u = u + g[..., t * m:(t + 1) * m]
    return u


def analysis_ref(x: np.ndarray, h: np.ndarray, m: int, hop: int, lead: int, frames: int, bins: int) -> np.ndarray:
    """[rows, frames, bins] complex64 of the [rows, nx] float32 array x."""
    from oracle import pyoracle

    assert 1 <= bins <= m
    u = fold(terms(x, h, hop, lead, frames), m)
    rows = u.shape[0]
    z = np.zeros((rows * frames, m), np.complex64)
    z.real = u.reshape(rows * frames, m)
    Z = pyoracle.fft_mt(z) if m > 1 and rows * frames else z
    return np.ascontiguousarray(Z.reshape(rows, frames, m)[:, :, :bins])


def complete(spec: np.ndarray, m: int) -> np.ndarray:
    """[..., bins] -> [..., M]: the frames as given (bins == M), or F[k] = (half[M-k].re, -half[M-k].im) for k >= bins = M/2 + 1."""
    bins = spec.shape[-1]
    if bins == m:
        return np.ascontiguousarray(spec, np.complex64)
    assert m % 2 == 0 and bins == m // 2 + 1
    full = np.empty(spec.shape[:-1] + (m,), np.complex64)
    full[..., :bins] = spec
    k = np.arange(bins, m)
    full[..., bins:].real = spec[..., m - k].real
    full[..., bins:].imag = -spec[..., m - k].imag
    return full


def inverse_ref(spec: np.ndarray, m: int) -> np.ndarray:
    """[rows, frames, bins] -> [rows, frames, M] float32: r_f = ifft(F_f).re"""
    from oracle import pyoracle

    rows, frames, _ = spec.shape
    full = complete(spec, m).reshape(rows * frames, m)
    v = pyoracle.fft_mt(full, inverse=True) if m > 1 and rows * frames else full
    return np.ascontiguousarray(v.real.reshape(rows, frames, m), F)


def synthesis_ref(spec: np.ndarray, g: np.ndarray, m: int, hop: int, scale) -> np.ndarray:
    """[rows, (frames - 1) D + nh] float32: the whole overlap-added result.  Per sample the terms are added in ascending frame order, the
    first one starting the accumulator; a sample that no frame covers is +0."""
    g = np.ascontiguousarray(g, F)
    nh = g.size
    rows, frames, _ = spec.shape
    r = inverse_ref(spec, m)
    scale = F(scale)
    full_len = (frames - 1) * hop + nh
    acc = np.zeros((rows, full_len), F)
    started = np.zeros(full_len, bool)
    idx = np.arange(nh)
    with np.errstate(invalid="ignore", over="ignore"):
        for f in range(frames):
            t = g[None, :] * r[:, f, idx % m]
            seg = slice(f * hop, f * hop + nh)
            first = ~started[seg]
            cur = acc[:, seg]
            acc[:, seg] = np.where(first[None, :], t, cur + t)
            started[seg] = True
        out = acc * scale
    out[:, ~started] = 0.0
    return out
