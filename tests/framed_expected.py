"""Expected values of every family call of a frame-geometry fuzz case (tests/framed_cases.py) from ONE pass of the CPU oracle's STFT per
row, for the largest frame count any family of the case asks for.  A frame's arithmetic does not depend on how many frames are
asked for, so every family's frames are a prefix of that pass: the full frames, their one-sided prefix, the magnitudes
(frontend_oracle.magnitudes' expression) and the row maximum, mel_oracle's energies and MFCCs, picture_oracle's pictures,
welch_oracle's grouped sums (with a second pass for the cross spectrum's second signal), onesided_ref's completion and
convolve_oracle's rows.  tests/test_framed_cases_cpu.py holds the shared pass to the per-family oracles.  Nothing here calls the
library."""
from __future__ import annotations

import numpy as np

import framed_cases as fc
import mel_oracle as mo
import onesided_ref
import picture_oracle as po
import welch_oracle as wo

F = np.float32


class Refused:
    """A call include/kofft_hip.h says is refused: the code, and an output that must stay untouched."""

    def __init__(self, code):
        self.code = code


def window_of(oracle, case, inp) -> np.ndarray:
    return oracle.hann(case.win_len) if inp["window"] is None else inp["window"]


def stft_pass(oracle, x: np.ndarray, win: np.ndarray, hop: int, frames: int) -> np.ndarray:
    """[rows, frames, win_len] complex64: oracle.stft of every row, once."""
    out = np.zeros((x.shape[0], frames, win.size), np.complex64)
    for r in range(x.shape[0]):
        out[r] = oracle.stft(x[r], win, hop, frames)
    return out


def magnitudes_of(S: np.ndarray, win_len: int) -> np.ndarray:
    """[rows, frames, win_len // 2] float32: sqrt(re * re + im * im), one multiply, one add, a correctly rounded root."""
    half = win_len // 2
    re, im = np.ascontiguousarray(S[..., :half].real, F), np.ascontiguousarray(S[..., :half].imag, F)
    with np.errstate(all="ignore"):
        return np.sqrt(re * re + im * im)


def welch_from(X: np.ndarray, Y, win_len: int, scale, double: bool, summed=wo.grouped_sum) -> np.ndarray:
    """[rows, K] from the rows' one-sided frames [rows, frames, K] (Y given: the cross spectrum)."""
    totals = [summed(wo._terms(X[r], None if Y is None else Y[r])) for r in range(X.shape[0])]
    return wo.finish(np.stack(totals), win_len, scale, double)


def expected(oracle, case, inp=None) -> dict:
    """family -> its expected output (a Refused where the header refuses the call).  Also "S" (the pass), "half" ([rows, frames, K] of the
    one-sided family) and "full" (its completion, the input of istft_parallel_rows)."""
    inp = fc.inputs(case) if inp is None else inp
    w, hop, rows = case.win_len, case.hop, case.rows
    K, half = w // 2 + 1, w // 2
    win = window_of(oracle, case, inp)
    most = max([case.required, 1] + list(case.frames.values()))
    S = stft_pass(oracle, inp["x"], win, hop, most)
    mags = magnitudes_of(S, w)
    out = {"S": S, "window": win}
    for fam, frames in case.frames.items():
        code = fc.refusal(case, fam)
        if code is not None:
            out[fam] = Refused(code)
            continue
        if fam == "stft":
            out[fam] = np.ascontiguousarray(S[:, :frames])
        elif fam == "onesided":
            out[fam] = np.ascontiguousarray(S[:, :frames, :K])
        elif fam == "mags":
            m = np.ascontiguousarray(mags[:, :frames])
            out[fam] = (m, np.array([po.row_max(m[r]) for r in range(rows)], F))
        elif fam == "mel":
            out[fam] = mo.energies(mags[:, :frames].reshape(rows * frames, half), inp["bins"]).reshape(rows, frames, case.num_mel)
        elif fam == "mfcc":
            out[fam] = mo.mfcc(mags[:, :frames].reshape(rows * frames, half), inp["bins"], case.num_coeffs).reshape(rows, frames, case.num_coeffs)
        elif fam == "picture":
            p = case.picture
            if half == 0:  # no bins: nothing written but max_out
                mx = {0: np.zeros(rows, F), 1: np.full(rows, po.SEED, F), 2: inp["max_in"]}[p["max_mode"]]
                out[fam] = (np.zeros(0, np.uint8), mx)
            else:
                out[fam] = po.pictures(np.ascontiguousarray(mags[:, :frames]), max_in=inp["max_in"], table=inp["table"], **p)
        elif fam == "welch":
            out[fam] = welch_from(S[:, :frames, :K], None, w, case.welch_scale, case.welch_double)
        elif fam == "csd":
            Sy = stft_pass(oracle, inp["y"], win, hop, max(case.required, frames, 1))
            out[fam] = welch_from(S[:, :frames, :K], Sy[:, :frames, :K], w, case.welch_scale, case.welch_double)
    if isinstance(out.get("onesided"), np.ndarray):
        out["half"] = out["onesided"]
        out["full"] = onesided_ref.complete(out["onesided"], w)
    return out


def conv_expected(c, inp=None) -> np.ndarray:
    """[rows, out_len]: convolve_ref's rows cut to the case's window."""
    from convolve_oracle import convolve_ref

    inp = fc.conv_inputs(c) if inp is None else inp
    full = convolve_ref(inp["x"], inp["h"], c.block, c.correlate)
    return np.ascontiguousarray(full[:, c.out_first:c.out_first + c.out_len])


def float64_frame(x_row: np.ndarray, win: np.ndarray, hop: int, f: int) -> np.ndarray:
    """numpy.fft.rfft of frame f of one row in float64: the windowed samples, zeros past the end of the row."""
    n = win.size
    seg = np.zeros(n, np.float64)
    part = x_row[f * hop:f * hop + n].astype(np.float64)
    seg[:part.size] = part
    return np.fft.rfft(seg * win.astype(np.float64))


def float64_pairs(case, count: int = 8) -> list:
    """Up to `count` (row, frame) pairs of frames that hold samples, from the case's own rng."""
    holding = min(case.frames.get("onesided", 0), fc.welch_frames_walked(case.len, case.hop, 1 << 62)) if case.len else 0
    if holding == 0:
        return []
    rng = np.random.default_rng(case.data_seed + 2)
    pairs = {(int(rng.integers(0, case.rows)), int(rng.integers(0, holding))) for _ in range(count)}
    return sorted(pairs)


def float64_errors(case, inp, win, onesided: np.ndarray) -> list:
    """The relative L2 error of [rows, frames, K] one-sided frames against float64_frame at float64_pairs."""
    errs = []
    for r, f in float64_pairs(case):
        want = float64_frame(inp["x"][r], win, case.hop, f)
        den = float(np.linalg.norm(want))
        if den > 0:
            errs.append(float(np.linalg.norm(onesided[r, f].astype(np.complex128) - want)) / den)
    return errs


# ---- the float64 bounds (measured in tests/test_framed_cases_cpu.py, whose docstring holds the table) ------------------------------
# win_len -> the measured maximum
MEASURED = {1: 4.22e-08, 2: 4.92e-08, 3: 2.22e-07, 5: 2.52e-07, 15: 1.6e-06, 16: 6.98e-08, 31: 2e-06, 32: 4.52e-07, 33: 2.92e-06,
            64: 3.35e-07, 128: 6.39e-07, 256: 5.69e-07, 400: 4.67e-05, 512: 1.08e-05, 1000: 7.73e-05, 1024: 1.51e-05,
            2048: 7.92e-06, 4096: 9.4e-05, 8192: 4.82e-05}


def float64_bound(win_len: int):
    return 2.5 * MEASURED[win_len] if win_len in MEASURED else None


def conv_float64_bound(block: int) -> float:
    return 1e-6 + 2e-7 * block  # tests/test_convolve_cpu.py


CONV_FLOAT64_MIN_VALUES = 8


def conv_float64_error(c, inp, got64: np.ndarray, first: int = 0):
    """The error of columns [first, first + got64.shape[1]) of the rows against numpy.convolve / numpy.correlate(.., "full") in float64,
    relative to the full rows: the L2 norm of the difference over the L2 norm of the whole float64 result scaled to the window's share
    of the values, sqrt(window / full) -- for the full rows the plain relative L2 error that tests/test_convolve_cpu.py bounds.  The
    window's own norm is no yardstick: the result passes through zero, and the error of overlap-save is the round-off of whole blocks,
    not of the value it lands on.  A window of fewer than CONV_FLOAT64_MIN_VALUES values per row (the last sample alone) has no
    meaningful relative error at all -- one value's error is several times the root mean square as often as not -- and gives None:
    such a window is held bit for bit to the oracle, whose full rows the CPU test bounds."""
    count = got64.shape[1]
    if count < min(CONV_FLOAT64_MIN_VALUES, c.full):
        return None
    x64 = inp["x"].astype(np.float64)
    h64 = inp["h"].astype(np.float64).reshape(-1, c.nh)
    op = (lambda a, b: np.correlate(a, b, "full")) if c.correlate else np.convolve
    want = np.stack([op(x64[r], h64[r if h64.shape[0] > 1 else 0]) for r in range(c.rows)])
    den = float(np.linalg.norm(want)) * np.sqrt(count / c.full)
    diff = float(np.linalg.norm(got64 - want[:, first:first + count]))
    return diff / den if den else diff
