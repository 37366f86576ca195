"""Test oracle of the Hartley transform (hartley.rs:12-57), written apart from kofft_amd/csrc/libm_trigf.hip.h: the libm crate's
sinf / cosf (the musl / FreeBSD s_sinf.c, s_cosf.c, k_sinf.c, k_cosf.c, e_rem_pio2f.c algorithm) restated in float64 numpy -- every
numpy operation on float64 arrays is one IEEE rounding, the final astype(float32) rounds to nearest even -- the table
H[i][k] = cosf(a) + sinf(a) and the +0-seeded f32 sums in increasing i.  Finite |x| >= 0x4dc90fdb (rem_pio2_large) is refused."""
import numpy as np

F = np.float32
_h = float.fromhex
S1, S2, S3, S4 = _h("-0x15555554cbac77p-55"), _h("0x111110896efbb2p-59"), _h("-0x1a00f9e2cae774p-65"), _h("0x16cd878c3b46a7p-71")
C0, C1, C2, C3 = _h("-0x1ffffffd0c5e81p-54"), _h("0x155553e1053a42p-57"), _h("-0x16c087e80f1e27p-62"), _h("0x199342e0ee5069p-68")
TOINT = 1.5 * 2.0 ** 52
INV_PIO2 = 6.36619772367581382433e-01
PIO2_1 = 1.57079631090164184570e+00
PIO2_1T = 1.58932547735281966916e-08
FRAC_PI_2 = float(np.pi) / 2.0  # core::f64::consts::FRAC_PI_2 (halving is exact)
P1, P2, P3, P4 = 1.0 * FRAC_PI_2, 2.0 * FRAC_PI_2, 3.0 * FRAC_PI_2, 4.0 * FRAC_PI_2

# the branch bounds of sinf.rs / cosf.rs (bit patterns of |x|) and the end of rem_pio2f's medium range
BOUNDS = (0x39800000, 0x3f490fda, 0x4016cbe3, 0x407b53d1, 0x40afeddf, 0x40e231d5)
MEDIUM_END = 0x4dc90fdb


def k_sinf(x):
    z = x * x
    w = z * z
    r = S3 + z * S4
    s = z * x
    return ((x + s * (S1 + z * S2)) + s * w * r).astype(F)


def k_cosf(x):
    z = x * x
    w = z * z
    r = C2 + z * C3
    return (((1.0 + z * C0) + w * C1) + (w * z) * r).astype(F)


def _split(x):
    x = np.ascontiguousarray(x, F)
    bits = x.view(np.uint32)
    ix = bits & np.uint32(0x7fffffff)
    if np.any((ix >= MEDIUM_END) & (ix < 0x7f800000)):
        raise ValueError("a finite |x| >= 0x4dc90fdb needs rem_pio2_large, which is not restated")
    return x, (bits >> np.uint32(31)) != 0, ix, x.astype(np.float64)


def _reduce(x64):
    fn = (x64 * INV_PIO2 + TOINT) - TOINT
    return fn.astype(np.int64) & 3, (x64 - fn * PIO2_1) - fn * PIO2_1T


def _select(shape, cases):
    """out[mask] = fn() for every (mask, fn) whose mask has a lane; the masks are disjoint and cover everything."""
    out = np.empty(shape, F)
    seen = np.zeros(shape, bool)
    for mask, fn in cases:
        if mask.any():
            out[mask] = fn(mask)
        seen |= mask
    assert seen.all()
    return out


def sinf(x):
    x, sg, ix, d = _split(x)
    with np.errstate(all="ignore"):
        big = (ix > 0x40e231d5) & (ix < 0x7f800000)
        q, y = _reduce(np.where(big, d, 0.0))
        return _select(x.shape, [
            (ix < 0x39800000, lambda m: x[m]),
            ((ix >= 0x39800000) & (ix <= 0x3f490fda), lambda m: k_sinf(d[m])),
            ((ix > 0x3f490fda) & (ix <= 0x4016cbe3) & sg, lambda m: -k_cosf(d[m] + P1)),
            ((ix > 0x3f490fda) & (ix <= 0x4016cbe3) & ~sg, lambda m: k_cosf(d[m] - P1)),
            ((ix > 0x4016cbe3) & (ix <= 0x407b53d1) & sg, lambda m: k_sinf(-(d[m] + P2))),
            ((ix > 0x4016cbe3) & (ix <= 0x407b53d1) & ~sg, lambda m: k_sinf(-(d[m] - P2))),
            ((ix > 0x407b53d1) & (ix <= 0x40afeddf) & sg, lambda m: k_cosf(d[m] + P3)),
            ((ix > 0x407b53d1) & (ix <= 0x40afeddf) & ~sg, lambda m: -k_cosf(d[m] - P3)),
            ((ix > 0x40afeddf) & (ix <= 0x40e231d5) & sg, lambda m: k_sinf(d[m] + P4)),
            ((ix > 0x40afeddf) & (ix <= 0x40e231d5) & ~sg, lambda m: k_sinf(d[m] - P4)),
            (ix >= 0x7f800000, lambda m: x[m] - x[m]),
            (big & (q == 0), lambda m: k_sinf(y[m])),
            (big & (q == 1), lambda m: k_cosf(y[m])),
            (big & (q == 2), lambda m: k_sinf(-y[m])),
            (big & (q == 3), lambda m: -k_cosf(y[m])),
        ])


def cosf(x):
    x, sg, ix, d = _split(x)
    with np.errstate(all="ignore"):
        big = (ix > 0x40e231d5) & (ix < 0x7f800000)
        q, y = _reduce(np.where(big, d, 0.0))
        return _select(x.shape, [
            (ix < 0x39800000, lambda m: np.ones(int(m.sum()), F)),
            ((ix >= 0x39800000) & (ix <= 0x3f490fda), lambda m: k_cosf(d[m])),
            ((ix > 0x3f490fda) & (ix <= 0x4016cbe3) & sg, lambda m: k_sinf(d[m] + P1)),
            ((ix > 0x3f490fda) & (ix <= 0x4016cbe3) & ~sg, lambda m: k_sinf(P1 - d[m])),
            ((ix > 0x4016cbe3) & (ix <= 0x407b53d1) & sg, lambda m: -k_cosf(d[m] + P2)),
            ((ix > 0x4016cbe3) & (ix <= 0x407b53d1) & ~sg, lambda m: -k_cosf(d[m] - P2)),
            ((ix > 0x407b53d1) & (ix <= 0x40afeddf) & sg, lambda m: k_sinf(-d[m] - P3)),
            ((ix > 0x407b53d1) & (ix <= 0x40afeddf) & ~sg, lambda m: k_sinf(d[m] - P3)),
            ((ix > 0x40afeddf) & (ix <= 0x40e231d5) & sg, lambda m: k_cosf(d[m] + P4)),
            ((ix > 0x40afeddf) & (ix <= 0x40e231d5) & ~sg, lambda m: k_cosf(d[m] - P4)),
            (ix >= 0x7f800000, lambda m: x[m] - x[m]),
            (big & (q == 0), lambda m: k_cosf(y[m])),
            (big & (q == 1), lambda m: k_sinf(-y[m])),
            (big & (q == 2), lambda m: -k_cosf(y[m])),
            (big & (q == 3), lambda m: k_sinf(y[m])),
        ])


def angles(n, rows=None, cols=None):
    """a[i][k] = factor * ((i * k) as f32), factor = (2.0 * PI) / n as f32 (hartley.rs:15, 19); rows / cols: the i / k to build."""
    i = np.arange(n, dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
    k = np.arange(n, dtype=np.int64) if cols is None else np.asarray(cols, np.int64)
    with np.errstate(all="ignore"):
        factor = (F(2.0) * F(np.pi)) / F(n)
        return factor * (i[:, None] * k[None, :]).astype(F)


_tables = {}


def table(n, rows=None, cols=None):
    """H[i][k] = cosf(a) + sinf(a), one f32 add (hartley.rs:20-22).  The whole table of a length is computed once and kept; with rows
    or cols only those entries are computed."""
    if rows is not None or cols is not None:
        a = angles(n, rows, cols)
        return cosf(a) + sinf(a)
    if n not in _tables:
        parts = []
        for r0 in range(0, n, 512):  # in slabs: the float64 temporaries of a large table would take gigabytes
            a = angles(n, range(r0, min(n, r0 + 512)))
            parts.append(cosf(a) + sinf(a))
        h = np.concatenate(parts) if parts else np.zeros((0, 0), F)
        h.setflags(write=False)
        _tables[n] = h
    return _tables[n]


def sample_cols(n, count, seed):
    """Sorted columns: both ends, both sides of every 128-column tile edge, and seeded others up to `count`."""
    cols = {0, n - 1} | {c for e in range(128, n, 128) for c in (e - 1, e)}
    rng = np.random.default_rng(seed)
    while len(cols) < min(count, n):
        cols.add(int(rng.integers(0, n)))
    return sorted(cols)


def dht(x, h=None, cols=None):
    """hartley::dht of every row of a [batch, n] float32 array: sum seeded with +0, i ascending, one f32 multiply and one f32 add
    per term.  h: the table to use (default: this oracle's); cols: only these outputs k (h, if given, holds those columns)."""
    x = np.ascontiguousarray(x, F)
    batch, n = x.shape
    if h is None:
        h = table(n) if cols is None else table(n, None, cols)
    acc = np.zeros((batch, h.shape[1] if n else 0), F)
    with np.errstate(all="ignore"):
        for i in range(n):
            acc = acc + x[:, i:i + 1] * h[i][None, :]
    return acc
