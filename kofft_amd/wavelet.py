"""kofft::wavelet (wavelet.rs:12-117, 154-567): haar, db2, db4, sym4 and coif1 wavelet transforms of f32 signals on the device, the
reference's arithmetic bit for bit.

``<name>_forward(input)`` returns (approx, detail), two new float32 arrays of len // 2; ``<name>_inverse(approx, detail)`` returns
2 * len(approx) samples (the detail must be at least as long as the approximation; extra entries are ignored, as in the reference).
``<name>_forward_multi(input, levels)`` / ``<name>_inverse_multi(approx, details)`` and the generic ``multi_level_forward`` /
``multi_level_inverse`` (and their ``_batch`` forms) follow wavelet.rs:54-117: an odd current row is padded with its last sample
before each level, details come finest first.  The generic functions run on the device when ``forward`` / ``inverse`` is one of this
module's functions, and run the reference's loop in Python around any other callable.  Lists of rows are grouped by length, one
device call per length.  ``fft=`` names the f32 HipFftImpl to run on; without one, a context on device 0 is created at the first
call and kept.  Errors are raised before any device is touched: a detail shorter than the approximation it is folded into raises
FftError(MismatchedLengths) (the reference panics there); rows over 2^26 samples or more than 64 levels raise DeviceError.

``cwt`` is the continuous counterpart (the reference has none): the scalogram of f32 rows against a bank of complex
wavelets, one per scale, by kofft_amd.convolve.correlate_bank in "same" mode.  ``morlet_taps`` samples the Morlet wavelets on the
host."""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

from .api import (WAVELET_MAX_LEN, WAVELET_MAX_LEVELS, DeviceError, FftError, HipFftImpl, dwt_multi_lengths, wavelet_id)

__all__ = ["haar_forward", "haar_inverse", "batch_forward", "batch_inverse", "multi_level_forward", "multi_level_inverse",
           "multi_level_forward_batch", "multi_level_inverse_batch", "db2_forward", "db2_inverse", "db2_forward_batch",
           "db2_inverse_batch", "db4_forward", "db4_inverse", "sym4_forward", "sym4_inverse", "coif1_forward", "coif1_inverse",
           "haar_forward_multi", "haar_inverse_multi", "db2_forward_multi", "db2_inverse_multi", "db4_forward_multi",
           "db4_inverse_multi", "sym4_forward_multi", "sym4_inverse_multi", "coif1_forward_multi", "coif1_inverse_multi",
           "morlet_taps", "cwt"]

_default: Optional[HipFftImpl] = None


def _ctx(fft: Optional[HipFftImpl]) -> HipFftImpl:
    global _default
    if fft is None:
        if _default is None:
            _default = HipFftImpl(np.float32)
        fft = _default
    return fft


def _row(x, name="input") -> np.ndarray:
    a = np.ascontiguousarray(x, np.float32)
    if a.ndim != 1:
        raise TypeError(f"{name} must be a 1-D signal")
    return a


def _check_len(n: int) -> None:
    if n > WAVELET_MAX_LEN:
        raise DeviceError(-2, f"wavelet rows take at most 2^26 samples")


def _check_levels(levels: int) -> int:
    levels = int(levels)
    if levels < 0:
        raise ValueError("levels is a usize in the reference: it cannot be negative")
    if levels > WAVELET_MAX_LEVELS:
        raise DeviceError(-2, f"at most {WAVELET_MAX_LEVELS} levels")
    return levels


def _empty():
    return np.empty(0, np.float32)


# ---- one level -----------------------------------------------------------------------------------------------------------------
def _forward_rows(w: int, rows: list, fft: Optional[HipFftImpl]) -> tuple:
    """(approx list, detail list) of 1-D float32 rows, one device call per length."""
    rows = [_row(r) for r in rows]
    for r in rows:
        _check_len(r.shape[0])
    groups: dict[int, list[int]] = {}
    for j, r in enumerate(rows):
        groups.setdefault(r.shape[0], []).append(j)
    avgs, diffs = [None] * len(rows), [None] * len(rows)
    for n, idx in groups.items():
        if n // 2 == 0:
            for j in idx:
                avgs[j], diffs[j] = _empty(), _empty()
            continue
        a, d = _ctx(fft).dwt_batch(np.stack([rows[j] for j in idx]), w)
        for t, j in enumerate(idx):
            avgs[j], diffs[j] = a[t], d[t]
    return avgs, diffs


def _inverse_rows(w: int, avgs: list, diffs: list, fft: Optional[HipFftImpl]) -> list:
    avgs = [_row(a, "approx") for a in avgs]
    diffs = [_row(d, "detail") for d in diffs]
    if len(avgs) != len(diffs):  # (zip in the reference stops at the shorter list)
        k = min(len(avgs), len(diffs))
        avgs, diffs = avgs[:k], diffs[:k]
    for a, d in zip(avgs, diffs):
        if d.shape[0] < a.shape[0]:
            raise FftError(FftError.MismatchedLengths)
        _check_len(2 * a.shape[0])
    groups: dict[int, list[int]] = {}
    for j, a in enumerate(avgs):
        groups.setdefault(a.shape[0], []).append(j)
    out = [None] * len(avgs)
    for n, idx in groups.items():
        if n == 0:
            for j in idx:
                out[j] = _empty()
            continue
        res = _ctx(fft).idwt_batch(np.stack([avgs[j] for j in idx]), np.stack([diffs[j][:n] for j in idx]), w)
        for t, j in enumerate(idx):
            out[j] = res[t]
    return out


def _forward(w: int, input, fft) -> tuple:
    a, d = _forward_rows(w, [input], fft)
    return a[0], d[0]


def _inverse(w: int, approx, detail, fft) -> np.ndarray:
    return _inverse_rows(w, [approx], [detail], fft)[0]


def haar_forward(input, fft: Optional[HipFftImpl] = None):
    """wavelet::haar_forward (wavelet.rs:12-21)."""
    return _forward(0, input, fft)


def haar_inverse(avg, diff, fft: Optional[HipFftImpl] = None):
    """wavelet::haar_inverse (wavelet.rs:24-33)."""
    return _inverse(0, avg, diff, fft)


def batch_forward(inputs, fft: Optional[HipFftImpl] = None):
    """wavelet::batch_forward (wavelet.rs:35-44): (avgs, diffs), lists of haar_forward's outputs."""
    return _forward_rows(0, list(inputs), fft)


def batch_inverse(avgs, diffs, fft: Optional[HipFftImpl] = None):
    """wavelet::batch_inverse (wavelet.rs:46-51)."""
    return _inverse_rows(0, list(avgs), list(diffs), fft)


def db2_forward(input, fft: Optional[HipFftImpl] = None):
    """wavelet::db2_forward (wavelet.rs:154-187)."""
    return _forward(1, input, fft)


def db2_inverse(approx, detail, fft: Optional[HipFftImpl] = None):
    """wavelet::db2_inverse (wavelet.rs:190-223): not a perfect round trip, as the reference says."""
    return _inverse(1, approx, detail, fft)


def db2_forward_batch(inputs, fft: Optional[HipFftImpl] = None):
    """wavelet::db2_forward_batch (wavelet.rs:244-253)."""
    return _forward_rows(1, list(inputs), fft)


def db2_inverse_batch(avgs, diffs, fft: Optional[HipFftImpl] = None):
    """wavelet::db2_inverse_batch (wavelet.rs:255-260)."""
    return _inverse_rows(1, list(avgs), list(diffs), fft)


def db4_forward(input, fft: Optional[HipFftImpl] = None):
    """wavelet::db4_forward (wavelet.rs:263-309)."""
    return _forward(2, input, fft)


def db4_inverse(approx, detail, fft: Optional[HipFftImpl] = None):
    """wavelet::db4_inverse (wavelet.rs:312-355)."""
    return _inverse(2, approx, detail, fft)


def sym4_forward(input, fft: Optional[HipFftImpl] = None):
    """wavelet::sym4_forward (wavelet.rs:358-403)."""
    return _forward(3, input, fft)


def sym4_inverse(approx, detail, fft: Optional[HipFftImpl] = None):
    """wavelet::sym4_inverse (wavelet.rs:406-449)."""
    return _inverse(3, approx, detail, fft)


def coif1_forward(input, fft: Optional[HipFftImpl] = None):
    """wavelet::coif1_forward (wavelet.rs:452-493)."""
    return _forward(4, input, fft)


def coif1_inverse(approx, detail, fft: Optional[HipFftImpl] = None):
    """wavelet::coif1_inverse (wavelet.rs:496-535)."""
    return _inverse(4, approx, detail, fft)


_FORWARD = {haar_forward: 0, db2_forward: 1, db4_forward: 2, sym4_forward: 3, coif1_forward: 4}
_INVERSE = {haar_inverse: 0, db2_inverse: 1, db4_inverse: 2, sym4_inverse: 3, coif1_inverse: 4}


# ---- multi level ---------------------------------------------------------------------------------------------------------------
def _python_forward(input, levels: int, forward: Callable) -> tuple:
    """multi_level_forward's loop (wavelet.rs:54-71) around a foreign single-level function."""
    current = np.array(input, np.float32).ravel()
    details = []
    for _ in range(levels):
        if current.shape[0] % 2 != 0 and current.shape[0] > 0:
            current = np.append(current, current[-1]).astype(np.float32)
        avg, diff = forward(current)
        details.append(diff)
        current = avg
    return current, details


def _multi_forward_rows(w: int, rows: list, levels: int, fft) -> tuple:
    rows = [_row(r) for r in rows]
    for r in rows:
        _check_len(r.shape[0])
    groups: dict[int, list[int]] = {}
    for j, r in enumerate(rows):
        groups.setdefault(r.shape[0], []).append(j)
    avgs, dets = [None] * len(rows), [None] * len(rows)
    for n, idx in groups.items():
        if n == 0:
            for j in idx:
                avgs[j], dets[j] = _empty(), [_empty() for _ in range(levels)]
            continue
        a, ds = _ctx(fft).wavedec_batch(np.stack([rows[j] for j in idx]), w, levels)
        for t, j in enumerate(idx):
            avgs[j], dets[j] = a[t].copy(), [d[t].copy() for d in ds]
    return avgs, dets


def _multi_inverse_rows(w: int, avgs: list, diffs: list, fft) -> list:
    avgs = [_row(a, "approx") for a in avgs]
    diffs = [[_row(d, "detail") for d in ds] for ds in diffs]
    k = min(len(avgs), len(diffs))
    avgs, diffs = avgs[:k], diffs[:k]
    for a, ds in zip(avgs, diffs):  # every error before the first call
        _check_levels(len(ds))
        cur = a.shape[0]
        if cur == 0:
            continue
        for d in reversed(ds):
            if d.shape[0] < cur:
                raise FftError(FftError.MismatchedLengths)
            cur *= 2
            _check_len(cur)
    groups: dict[tuple, list[int]] = {}
    for j, (a, ds) in enumerate(zip(avgs, diffs)):
        groups.setdefault((a.shape[0], tuple(d.shape[0] for d in ds)), []).append(j)
    out = [None] * k
    for (n, dl), idx in groups.items():
        if n == 0:
            for j in idx:
                out[j] = _empty()
            continue
        res = _ctx(fft).waverec_batch(np.stack([avgs[j] for j in idx]),
                                      [np.stack([diffs[j][l] for j in idx]) for l in range(len(dl))], w)
        for t, j in enumerate(idx):
            out[j] = res[t]
    return out


def multi_level_forward(input, levels: int, forward: Callable, fft: Optional[HipFftImpl] = None):
    """wavelet::multi_level_forward (wavelet.rs:54-71): (approx, [detail_1 .. detail_L]), finest first."""
    levels = _check_levels(levels)
    w = _FORWARD.get(forward)
    if w is None:
        return _python_forward(input, levels, forward)
    a, d = _multi_forward_rows(w, [input], levels, fft)
    return a[0], d[0]


def multi_level_inverse(approx, details, inverse: Callable, fft: Optional[HipFftImpl] = None):
    """wavelet::multi_level_inverse (wavelet.rs:74-83): the details folded in from the coarsest to the finest."""
    w = _INVERSE.get(inverse)
    if w is None:
        current = np.array(approx, np.float32).ravel()
        for d in reversed(list(details)):
            current = inverse(current, d)
        return current
    return _multi_inverse_rows(w, [approx], [list(details)], fft)[0]


def multi_level_forward_batch(inputs, levels: int, forward: Callable, fft: Optional[HipFftImpl] = None):
    """wavelet::multi_level_forward_batch (wavelet.rs:86-102): (avgs, [details per input])."""
    levels = _check_levels(levels)
    w = _FORWARD.get(forward)
    if w is None:
        res = [_python_forward(x, levels, forward) for x in inputs]
        return [r[0] for r in res], [r[1] for r in res]
    return _multi_forward_rows(w, list(inputs), levels, fft)


def multi_level_inverse_batch(avgs, diffs, inverse: Callable, fft: Optional[HipFftImpl] = None):
    """wavelet::multi_level_inverse_batch (wavelet.rs:105-117)."""
    w = _INVERSE.get(inverse)
    if w is None:
        return [multi_level_inverse(a, d, inverse) for a, d in zip(avgs, diffs)]
    return _multi_inverse_rows(w, list(avgs), [list(d) for d in diffs], fft)


def _multi(w: int):
    fwd = {0: haar_forward, 1: db2_forward, 2: db4_forward, 3: sym4_forward, 4: coif1_forward}[w]
    inv = {0: haar_inverse, 1: db2_inverse, 2: db4_inverse, 3: sym4_inverse, 4: coif1_inverse}[w]

    def forward_multi(input, levels: int, fft: Optional[HipFftImpl] = None):
        return multi_level_forward(input, levels, fwd, fft)

    def inverse_multi(avg, details, fft: Optional[HipFftImpl] = None):
        return multi_level_inverse(avg, details, inv, fft)

    return forward_multi, inverse_multi


# wavelet.rs:538-567
haar_forward_multi, haar_inverse_multi = _multi(0)
db2_forward_multi, db2_inverse_multi = _multi(1)
db4_forward_multi, db4_inverse_multi = _multi(2)
sym4_forward_multi, sym4_inverse_multi = _multi(3)
coif1_forward_multi, coif1_inverse_multi = _multi(4)
for _name in ("haar", "db2", "db4", "sym4", "coif1"):
    globals()[f"{_name}_forward_multi"].__name__ = f"{_name}_forward_multi"
    globals()[f"{_name}_inverse_multi"].__name__ = f"{_name}_inverse_multi"
    globals()[f"{_name}_forward_multi"].__doc__ = f"wavelet::{_name}_forward_multi: multi_level_forward with {_name}_forward."
    globals()[f"{_name}_inverse_multi"].__doc__ = f"wavelet::{_name}_inverse_multi: multi_level_inverse with {_name}_inverse."
del _name


# ---- continuous wavelet transform --------------------------------------------------------------------------------
def morlet_taps(scales, w0: float = 6.0, support: float = 4.0) -> np.ndarray:
    """complex64 [len(scales), nh] Morlet wavelets, one row per scale s (in samples), computed in float64: nh = 2 ceil(support
    max(scales)) + 1 taps at t = i - (nh - 1) / 2 of pi^(-1/4) exp(i w0 t / s) exp(-(t / s)^2 / 2) / sqrt(s), zero where |t| >
    ceil(support s).  Row s has its centre frequency at w0 / (2 pi s) cycles per sample."""
    sc = np.asarray(scales, np.float64)
    if sc.ndim != 1 or sc.size == 0:
        raise ValueError("scales must be a non-empty 1-D sequence")
    if not (np.isfinite(sc).all() and (sc > 0).all()) or not (np.isfinite(support) and support > 0) or not np.isfinite(w0):
        raise ValueError("scales and support must be positive and finite, w0 finite")
    half = int(np.ceil(support * sc.max()))
    t = np.arange(-half, half + 1, dtype=np.float64)[None, :] / sc[:, None]
    taps = np.pi ** -0.25 * np.exp(1j * float(w0) * t) * np.exp(-0.5 * t * t) / np.sqrt(sc)[:, None]
    taps[np.abs(np.arange(-half, half + 1))[None, :] > np.ceil(support * sc)[:, None]] = 0.0
    return taps.astype(np.complex64)


def cwt(x, scales=None, w0: float = 6.0, support: float = 4.0, out: str = "magnitude", block: Optional[int] = None,
        fft: Optional[HipFftImpl] = None, taps=None) -> np.ndarray:
    """The scalogram of a 1-D signal or of every row of a 2-D [rows, nx] array: correlate_bank(x, morlet_taps(scales, w0, support),
    "same", block, out), [scales, nx] or [rows, scales, nx].  ``out``: "magnitude" (float32), "complex" (complex64) or "real"
    (float32).  ``taps=``: the caller's own [scales, nh] wavelets in place of ``scales`` (nh odd keeps them centred)."""
    from . import convolve

    if (scales is None) == (taps is None):
        raise ValueError("pass either scales or taps=")
    bank = morlet_taps(scales, w0, support) if taps is None else taps
    return convolve.correlate_bank(x, bank, "same", block, out, fft)
