"""Expected values of the audio front end (rows of samples -> mel energies / MFCCs): the two existing oracles composed.  The magnitudes
are oracle.stft_magnitudes' (window None, the frame count it produces); for a caller's window, or more frames than ceil(len / hop),
the oracle's STFT with that window followed by numpy float32 sqrt(re * re + im * im) of bins < win_len / 2 (one multiply, one add, a
correctly rounded root: the expression of visual/spectrogram.rs:63-66).  Then tests/mel_oracle.py.  Test infrastructure: nothing here
calls the library."""
from __future__ import annotations

import numpy as np

import mel_oracle as mo

F = np.float32


def magnitudes(oracle, x: np.ndarray, win_len: int, hop: int, frames: int, window=None) -> np.ndarray:
    """[rows, frames, win_len // 2] float32."""
    rows, length = x.shape
    half = win_len // 2
    out = np.zeros((rows, frames, half), F)
    required = -(-length // hop)
    for r in range(rows):
        if window is None and frames == required:
            out[r] = oracle.stft_magnitudes(x[r], win_len, hop)[0]
            continue
        win = oracle.hann(win_len) if window is None else np.ascontiguousarray(window, F)
        st = oracle.stft(x[r], win, hop, frames)[:, :half]
        re, im = np.ascontiguousarray(st.real, F), np.ascontiguousarray(st.imag, F)
        with np.errstate(all="ignore"):
            out[r] = np.sqrt(re * re + im * im)
    return out


def expected(oracle, x: np.ndarray, win_len: int, hop: int, frames: int, bins, window=None):
    """(energies [rows, frames, num_mel], coefficients [rows, frames, num_mel]): truncate the latter to num_coeffs columns."""
    rows = x.shape[0]
    num_mel = len(bins) - 2
    mags = magnitudes(oracle, x, win_len, hop, frames, window).reshape(rows * frames, win_len // 2)
    e = mo.energies(mags, bins)
    c = np.ascontiguousarray(mo.tdo.direct("dct", 2, mo.log_mel(e)))
    return e.reshape(rows, frames, num_mel), c.reshape(rows, frames, num_mel)


def signal(rng, rows: int, length: int, special: bool = True) -> np.ndarray:
    """N(0, 1) rows; with room: a stretch of +0 and -0, subnormals, one inf and one NaN sample (each poisons exactly the frames that
    cover it)."""
    x = rng.standard_normal((rows, length)).astype(F)
    if not special or length < 8:
        return x
    x[0, length // 4: length // 4 + max(1, length // 8)] = 0.0
    x[0, length // 4 + 1] = -0.0
    x[0, 1] = 1e-41
    x[0, 2] = -1e-45
    if rows > 1:
        x[1, length // 2] = np.inf
        x[1, :length // 3] = 0.0  # whole frames of silence where the hop is short
    if rows > 2:
        x[2, (2 * length) // 3] = np.nan
    else:
        x[0, length - 1] = np.nan
    return x
