"""Every row of a batch against the oracle, bit for bit, with a report that points at the rows: how many differ, the first few row
indices and, for each, the first differing element (its column, the two values and their bits).  A tile walk, a ragged last round or
a chunk seam shows as a run of row indices; a sample of rows does not see it."""
from __future__ import annotations

import numpy as np

_CHUNK_BYTES = 64 << 20  # rows compared per step: bounds the temporary masks on batches of hundreds of MiB
_SHOW = 8


def _words(a: np.ndarray) -> np.ndarray:
    """[rows, words] unsigned view of the element bits (complex: re and im as separate words)."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "c":
        a = a.view(a.real.dtype)
    u = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    rows = a.shape[0] if a.ndim >= 2 else 1
    return a.view(u).reshape(rows, -1), a.reshape(rows, -1)


def _row_diff(gw, ww, gv, wv, nan_safe):
    """[rows, words] bool: True where an element differs (nan_safe: NaN against NaN is equal whatever its sign and payload)."""
    diff = gw != ww
    if nan_safe and gv.dtype.kind == "f":
        diff &= ~(np.isnan(gv) & np.isnan(wv))
    return diff


def row_mismatches(got: np.ndarray, want: np.ndarray, nan_safe: bool = False) -> list[tuple[int, int]]:
    """(row, first differing word) of every row that differs."""
    gw, gv = _words(got)
    ww, wv = _words(want)
    rows, words = gw.shape
    step = max(1, _CHUNK_BYTES // max(1, words * gw.itemsize))
    bad: list[tuple[int, int]] = []
    for r0 in range(0, rows, step):
        d = _row_diff(gw[r0:r0 + step], ww[r0:r0 + step], gv[r0:r0 + step], wv[r0:r0 + step], nan_safe)
        for r in np.flatnonzero(d.any(axis=1)):
            bad.append((r0 + int(r), int(np.argmax(d[r]))))
    return bad


def assert_rows_equal(got, want, what: str = "", nan_safe: bool = False) -> None:
    """Every row of `got` (axis 0; a 1-D array is one row) the same bits as `want`'s.  nan_safe: NaNs in the same places count as
    equal whatever their sign (an Inf - Inf is the platform's default NaN, whose sign differs between x86 and gfx950)."""
    got = np.asarray(got)
    want = np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        raise AssertionError(f"{what}: got {got.dtype}{list(got.shape)}, want {want.dtype}{list(want.shape)}")
    if got.size == 0:
        return
    bad = row_mismatches(got, want, nan_safe)
    if not bad:
        return
    gw, gv = _words(got)
    ww, wv = _words(want)
    per = 2 if got.dtype.kind == "c" else 1
    lines = []
    for r, w in bad[:_SHOW]:
        part = "" if per == 1 else (".re", ".im")[w % 2]
        lines.append(f"  row {r} col {w // per}{part}: got {gv[r, w]} ({int(gw[r, w]):#x}) want {wv[r, w]} ({int(ww[r, w]):#x})")
    rows = gw.shape[0]
    raise AssertionError(f"{what}: {len(bad)} of {rows} rows differ, first at rows {[r for r, _ in bad[:_SHOW]]}\n" + "\n".join(lines))
