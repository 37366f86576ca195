"""kofft::window and kofft::window_more (window.rs:24-61, window_more.rs:13-64): the reference's windows as float32 arrays, generated
by the library's host recipes bit for bit -- every expression in f32 in Rust's parse order, glibc's cosf where the reference calls
``.cos()`` (hann, hamming, blackman, tukey), the libm crate's restated cosf / sinf where it imports them (bohman, nuttall).

Edge cases are the reference's: a length of 1 gives NaN where it divides zero by zero (bartlett, bohman, nuttall, kaiser);
``kaiser(0, beta)`` raises FftError(EmptyInput) (the reference underflows ``len - 1``); ``tukey`` clamps alpha to [0, 1], and a NaN
alpha, like alpha <= 0, gives all ones."""
from __future__ import annotations

import numpy as np

from .api import hann, make_window as window

__all__ = ["hann", "hamming", "blackman", "kaiser", "tukey", "bartlett", "bohman", "nuttall", "window"]


def hamming(length: int) -> np.ndarray:
    """window::hamming (window.rs:31-35)."""
    return window("hamming", length)


def blackman(length: int) -> np.ndarray:
    """window::blackman (window.rs:38-48)."""
    return window("blackman", length)


def kaiser(length: int, beta: float) -> np.ndarray:
    """window::kaiser (window.rs:52-61)."""
    return window("kaiser", length, beta)


def tukey(length: int, alpha: float) -> np.ndarray:
    """window_more::tukey (window_more.rs:13-28)."""
    return window("tukey", length, alpha)


def bartlett(length: int) -> np.ndarray:
    """window_more::bartlett (window_more.rs:31-39)."""
    return window("bartlett", length)


def bohman(length: int) -> np.ndarray:
    """window_more::bohman (window_more.rs:42-50)."""
    return window("bohman", length)


def nuttall(length: int) -> np.ndarray:
    """window_more::nuttall (window_more.rs:53-64)."""
    return window("nuttall", length)
