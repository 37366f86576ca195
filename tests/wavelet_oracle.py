"""The reference's wavelet.rs restated with numpy float32, vectorised over the rows of a batch; independent of the library.

Every function takes a 2-D [batch, len] float32 array (or a list of them for the details) and returns float32 arrays.  The
arithmetic is the reference's, operation for operation: numpy float32 `*` and `+` are single IEEE operations (never fused).
  forward   haar (x[j] + x[j+1]) / 2.0; db2 h0*r(j) + h1*r(j+1) + h2*r(j+2) + h3*r(j+3) left to right (not seeded); db4 / sym4 /
            coif1 acc = +0.0, acc += h[k] * r(j+k), k ascending; r() the `while` reflection over the input length.
  inverse   haar a + d / a - d; the others out = +0.0, out[r(2i+k)] += (g[k] * a[i] + h[k] * d[i]) over (i, k) in lexicographic
            order: the direct hits in ascending i for every output, then the outputs a reflected hit can reach (the last L - 1, and
            every output of a row shorter than L) recomputed by scanning (i, k) in order.
  multi     an odd current row is padded with its last sample before each level; the inverse folds details coarsest first and
            raises MismatchedLengths where the reference indexes past a detail's end."""
from __future__ import annotations

import numpy as np

F = np.float32
NAMES = ("haar", "db2", "db4", "sym4", "coif1")

# the reference's decimal strings, wavelet.rs (forward: h, g; inverse: g multiplies the approximation, h the detail)
DECIMALS = {
    ("db2", False): (["0.4829629131445341", "0.8365163037378079", "0.2241438680420134", "-0.1294095225512604"],
                     ["-0.1294095225512604", "-0.2241438680420134", "0.8365163037378079", "-0.4829629131445341"]),
    ("db2", True): (["0.4829629131445341", "0.8365163037378079", "0.2241438680420134", "-0.1294095225512604"],
                    ["-0.1294095225512604", "-0.2241438680420134", "0.8365163037378079", "-0.4829629131445341"]),
    ("db4", False): (["-0.010597401785069032", "0.0328830116668852", "0.030841381835560764", "-0.18703481171909309",
                      "-0.027983769416859854", "0.6308807679298589", "0.7148465705529157", "0.2303778133088965"],
                     ["-0.2303778133088965", "0.7148465705529157", "-0.6308807679298589", "-0.027983769416859854",
                      "0.18703481171909309", "0.030841381835560764", "-0.0328830116668852", "-0.010597401785069032"]),
    ("db4", True): (["0.2303778133088965", "0.7148465705529157", "0.6308807679298589", "-0.027983769416859854",
                     "-0.18703481171909309", "0.030841381835560764", "0.0328830116668852", "-0.010597401785069032"],
                    ["-0.010597401785069032", "-0.0328830116668852", "0.030841381835560764", "0.18703481171909309",
                     "-0.027983769416859854", "-0.6308807679298589", "0.7148465705529157", "-0.2303778133088965"]),
    ("sym4", False): (["-0.07576571478927333", "-0.02963552764599851", "0.49761866763201545", "0.8037387518059161",
                       "0.29785779560527736", "-0.09921954357684722", "-0.012603967262037833", "0.0322231006040427"],
                      ["-0.0322231006040427", "-0.012603967262037833", "0.09921954357684722", "0.29785779560527736",
                       "-0.8037387518059161", "0.49761866763201545", "0.02963552764599851", "-0.07576571478927333"]),
    ("sym4", True): (["0.0322231006040427", "-0.012603967262037833", "-0.09921954357684722", "0.29785779560527736",
                      "0.8037387518059161", "0.49761866763201545", "-0.02963552764599851", "-0.07576571478927333"],
                     ["-0.07576571478927333", "0.02963552764599851", "0.49761866763201545", "-0.8037387518059161",
                      "0.29785779560527736", "0.09921954357684722", "-0.012603967262037833", "-0.0322231006040427"]),
    ("coif1", False): (["-0.015655728135791993", "-0.07273261951252645", "0.3848648468648578", "0.8525720202116004",
                        "0.3378976624574818", "-0.07273261951252645"],
                       ["0.07273261951252645", "0.3378976624574818", "-0.8525720202116004", "0.3848648468648578",
                        "0.07273261951252645", "-0.015655728135791993"]),
    ("coif1", True): (["-0.07273261951252645", "0.3378976624574818", "0.8525720202116004", "0.3848648468648578",
                       "-0.07273261951252645", "-0.015655728135791993"],
                      ["-0.015655728135791993", "0.07273261951252645", "0.3848648468648578", "-0.8525720202116004",
                       "0.3378976624574818", "0.07273261951252645"]),
}


def taps(name: str, inverse: bool):
    """(lo, hi) float32 arrays: Python parses each decimal to the nearest double and numpy rounds that to float32 -- checked against
    the correctly rounded f32 of the decimal by the CPU tests."""
    lo, hi = DECIMALS[(name, inverse)]
    return np.array([float(v) for v in lo], F), np.array([float(v) for v in hi], F)


def ntaps(name: str) -> int:
    return 2 if name == "haar" else len(DECIMALS[(name, False)][0])


def reflect(idx: np.ndarray, length: int) -> np.ndarray:
    """The reference's `while` loop, elementwise (length >= 2)."""
    idx = np.array(idx, np.int64)
    while True:
        neg, big = idx < 0, idx >= length
        if not (neg.any() or big.any()):
            return idx
        idx = np.where(neg, -idx, np.where(big, 2 * (length - 1) - idx, idx))


def forward(name: str, x: np.ndarray):
    """<name>_forward on every row: (approx, detail), [batch, len // 2] each."""
    x = np.asarray(x, F)
    b, length = x.shape
    n = length // 2
    if n == 0:
        return np.zeros((b, 0), F), np.zeros((b, 0), F)
    j = 2 * np.arange(n)
    if name == "haar":
        x0, x1 = x[:, j], x[:, j + 1]
        return (x0 + x1) / F(2.0), (x0 - x1) / F(2.0)
    h, g = taps(name, False)
    cols = [x[:, reflect(j + k, length)] for k in range(len(h))]
    if name == "db2":
        a = h[0] * cols[0] + h[1] * cols[1] + h[2] * cols[2] + h[3] * cols[3]
        d = g[0] * cols[0] + g[1] * cols[1] + g[2] * cols[2] + g[3] * cols[3]
        return a, d
    a = np.zeros((b, n), F)
    d = np.zeros((b, n), F)
    for k in range(len(h)):
        a = a + h[k] * cols[k]
        d = d + g[k] * cols[k]
    return a, d


def inverse(name: str, a: np.ndarray, d: np.ndarray) -> np.ndarray:
    """<name>_inverse on every row: [batch, n] approximations, [batch, >= n] details -> [batch, 2n]."""
    a = np.asarray(a, F)
    b, n = a.shape
    d = np.asarray(d, F)[:, :n]
    length = 2 * n
    out = np.zeros((b, length), F)
    if n == 0:
        return out
    if name == "haar":
        out[:, 0::2] = a + d
        out[:, 1::2] = a - d
        return out
    g, h = taps(name, True)
    L = len(g)
    H = L // 2
    p = np.arange(length)
    m, par = p // 2, p % 2
    for s in range(H):  # direct hits, ascending i
        i = m - (H - 1) + s
        k = par + 2 * (H - 1 - s)
        ok = (i >= 0) & (i < n)
        ii, kk = np.where(ok, i, 0), np.where(ok, k, 0)
        term = g[kk] * a[:, ii] + h[kk] * d[:, ii]
        out = np.where(ok, out + term, out)
    tail = range(0, length) if length < L else range(length - L + 1, length)
    i_start = (length - 2 * L) // 2 if length >= 2 * L else 0
    for q in tail:  # outputs a reflected hit can reach: every (i, k) in order
        acc = np.zeros(b, F)
        for i in range(i_start, n):
            for k in range(L):
                if int(reflect(2 * i + k, length)) == q:
                    acc = acc + (g[k] * a[:, i] + h[k] * d[:, i])
        out[:, q] = acc
    return out


def multi_lengths(length: int, levels: int) -> list:
    out = [length]
    for _ in range(levels):
        out.append((out[-1] + 1) // 2)
    return out


def forward_multi(name: str, x: np.ndarray, levels: int):
    """multi_level_forward with <name>_forward on every row: (approx, [detail_1 .. detail_L])."""
    cur = np.asarray(x, F)
    details = []
    for _ in range(levels):
        if cur.shape[1] % 2 == 1:
            cur = np.concatenate([cur, cur[:, -1:]], axis=1)
        cur, det = forward(name, cur)
        details.append(det)
    return cur, details


class MismatchedLengths(Exception):
    pass


def inverse_multi(name: str, a: np.ndarray, details: list) -> np.ndarray:
    """multi_level_inverse with <name>_inverse on every row (details finest first)."""
    cur = np.asarray(a, F)
    for det in reversed(details):
        if cur.shape[1] and det.shape[1] < cur.shape[1]:
            raise MismatchedLengths()
        cur = inverse(name, cur, det)
    return cur
