"""Expected values of the Welch power spectra and cross spectra of rows, composed from the CPU oracle: the frames of
pyoracle.stft_mt per row, bins < K = win_len // 2 + 1; the products and the two-level sums (groups of 32 frames, then the groups'
partials, both ascending from +0) as numpy float32 array operations over the bin axis, one frame at a time -- exact IEEE, nothing
fused; the complex product on the .real and .imag views (numpy's complex64 multiply may fuse or reorder)."""
from __future__ import annotations

import numpy as np

GROUP = 32  # KOFFT_HIP_WELCH_GROUP
F = np.float32


# the group-edge grid of tests/test_gpu_welch.py; tests/test_welch_cpu.py checks on the CPU that its 33- and 65-frame inputs tell the
# grouped order from a flat one
GRID_WINS = (32, 64, 256, 1024, 4096)
GRID_FRAMES = (1, 31, 32, 33, 65)
GRID_ROWS = (1, 3)


def grid_hops(win_len: int):
    return (win_len // 4, win_len, win_len + 3) + ((1,) if win_len == 64 else ())


def grid_input(win_len: int, hop: int, frames: int, rows: int, which: int = 0) -> np.ndarray:
    """[rows, len] N(0, 1) float32 whose last frame runs three samples past the end of the row."""
    length = max(1, (frames - 1) * hop + win_len - 3)
    rng = np.random.default_rng(26000 + 7 * win_len + 3 * hop + 11 * frames + rows + 100003 * which)
    return rng.standard_normal((rows, length)).astype(F)


def frames_of(row: np.ndarray, window: np.ndarray, hop: int, frames: int) -> np.ndarray:
    """[frames, K] complex64: bins < K of stft::stft's frames 0 .. frames - 1 of one row (frames past the row are transforms of +0)."""
    from oracle import pyoracle

    row = np.ascontiguousarray(row, F)
    win_len = window.size
    # stft_mt wants frames >= ceil(len / hop): a row cut after the last sample the wanted frames read, and as many frames as that needs
    seen = row[:min(row.size, (frames - 1) * hop + win_len)]
    need = max(frames, -(-seen.size // hop))
    return np.ascontiguousarray(pyoracle.stft_mt(seen, window, hop, need)[:frames, :win_len // 2 + 1])


def _terms(X: np.ndarray, Y) -> np.ndarray:
    """[frames, K] float32 |X|^2, or [frames, K] complex64 conj(X) Y."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if Y is None:
            return X.real * X.real + X.imag * X.imag
        c = np.empty_like(X)
        c.real = X.real * Y.real + X.imag * Y.imag
        c.imag = X.real * Y.imag - X.imag * Y.real
        return c


def _add(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore", over="ignore"):
        if a.dtype.kind != "c":
            return a + b
        out = np.empty_like(a)
        out.real = a.real + b.real
        out.imag = a.imag + b.imag
        return out


def grouped_sum(terms: np.ndarray, group: int = GROUP) -> np.ndarray:
    """The contract's order: partials of `group` consecutive frames ascending from +0, then the partials ascending from +0."""
    total = np.zeros(terms.shape[1], terms.dtype)
    for g0 in range(0, terms.shape[0], group):
        part = np.zeros(terms.shape[1], terms.dtype)
        for f in range(g0, min(g0 + group, terms.shape[0])):
            part = _add(part, terms[f])
        total = _add(total, part)
    return total


def flat_sum(terms: np.ndarray) -> np.ndarray:
    """What the contract is NOT: every frame ascending onto one sum."""
    return grouped_sum(terms, terms.shape[0] if terms.shape[0] else 1)


def _finish(total: np.ndarray, win_len: int, scale, double: bool) -> np.ndarray:
    K = win_len // 2 + 1
    s = F(scale)
    two = np.ones(K, F)
    if double:
        two[1:K if win_len % 2 else K - 1] = F(2.0)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if total.dtype.kind != "c":
            return (total * s) * two
        out = np.empty_like(total)
        out.real = (total.real * s) * two
        out.imag = (total.imag * s) * two
        return out


def welch_totals(x: np.ndarray, window: np.ndarray, hop: int, frames: int, y=None) -> np.ndarray:
    """[rows, K] float32 (y given: complex64, conj(X) Y): the rows' totals before the scale, of the [rows, len] float32 array x."""
    x = np.ascontiguousarray(x, F)
    window = np.ascontiguousarray(window, F)
    assert x.ndim == 2 and frames >= 1 and hop >= 1 and window.size >= 1
    rows = []
    for r in range(x.shape[0]):
        X = frames_of(x[r], window, hop, frames)
        Y = None if y is None else frames_of(y[r], window, hop, frames)
        rows.append(grouped_sum(_terms(X, Y)))
    return np.ascontiguousarray(np.stack(rows))


def finish(totals: np.ndarray, win_len: int, scale=1.0, double: bool = False) -> np.ndarray:
    """(total * scale) (* 2.0f on the interior bins) of every row of welch_totals' result."""
    return np.ascontiguousarray(np.stack([_finish(t, win_len, scale, double) for t in totals]))


def welch_ref(x: np.ndarray, window: np.ndarray, hop: int, frames: int, scale=1.0, double: bool = False, y=None) -> np.ndarray:
    """[rows, K] float32 (y given: complex64) as kofft_hip_welch_f32 / kofft_hip_csd_f32 define them."""
    return finish(welch_totals(x, window, hop, frames, y), np.asarray(window).size, scale, double)
