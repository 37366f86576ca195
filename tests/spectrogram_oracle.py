"""Expected values of visual::spectrogram's colour helpers (visual/spectrogram.rs:96-234) in numpy float32: every operation a float32
operation (numpy rounds each one), in the reference's order.  `log10` is the libm 0.2 crate's log10f (the musl / FreeBSD e_log10f.c
port), vectorised below as cepstrum_oracle does logf; `ln` in map_bin_to_pixel is glibc's logf through ctypes.  Written apart from the
device's restatement (kofft_amd/csrc/libm_log10f.hip.h, spectrogram_impl.hip.h): the two agreeing bit for bit is the second opinion.

Rust's rules restated here: f32::max (a NaN loses), f32::clamp (a NaN stays), `as u8` (truncating, saturating, NaN -> 0), f32::round
(half away from zero), Fire's first-matching-window search with its fallback to the last segment, Rainbow's strict `t >` walk."""
from __future__ import annotations

import ctypes as C

import numpy as np

from cepstrum_oracle import LG1, LG2, LG3, LG4

F = np.float32
_U = np.uint32


def _bits(v: int) -> np.float32:
    return np.array(v, _U).view(F)[()]


IVLN10HI, IVLN10LO, LOG10_2HI, LOG10_2LO = _bits(0x3EDE6000), _bits(0xB804EAD9), _bits(0x3E9A2080), _bits(0x355427DB)
FIRE, LEGACY, GRAY, VIRIDIS, PLASMA, INFERNO, RAINBOW = range(7)
IMPLEMENTED = (FIRE, LEGACY, GRAY, RAINBOW)
FIRE_STOPS = [(0.0, (0, 0, 0)), (0.25, (128, 0, 128)), (0.5, (255, 165, 0)), (0.75, (255, 255, 0)), (1.0, (255, 255, 255))]
RAINBOW_STOPS = [(0.0, (0, 0, 0)), (0.25, (0, 0, 255)), (0.5, (0, 255, 255)), (0.75, (255, 255, 0)), (0.9, (255, 0, 0)), (1.0, (255, 255, 255))]

_libm = C.CDLL("libm.so.6")
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]


def libm_log10f(x, log10=None) -> np.ndarray:
    """log10f of libm 0.2 on a float32 array.  (`log10`: another function to use instead -- the glibc twin of the record test.)"""
    x = np.array(x, F, copy=True, ndmin=1)
    if log10 is not None:
        with np.errstate(all="ignore"):
            return log10(x).astype(F)
    ix = x.view(_U).copy()
    k = np.zeros(x.shape, np.int32)
    out = np.zeros(x.shape, F)
    done = np.zeros(x.shape, bool)
    with np.errstate(all="ignore"):
        small_or_neg = (ix < _U(0x00800000)) | ((ix >> _U(31)) != 0)
        zero = small_or_neg & ((ix << _U(1)) == 0)
        out[zero] = F(-1.0) / (x[zero] * x[zero])
        done |= zero
        neg = small_or_neg & ~done
        neg &= (ix >> _U(31)) != 0
        out[neg] = (x[neg] - x[neg]) / F(0.0)
        done |= neg
        sub = small_or_neg & ~done
        k[sub] -= 25
        x[sub] = x[sub] * _bits(0x4C000000)
        ix[sub] = x[sub].view(_U)
        big = ~small_or_neg & (ix >= _U(0x7F800000))
        out[big] = x[big]
        done |= big
        one = ~small_or_neg & ~done & (ix == _U(0x3F800000))
        out[one] = F(0.0)
        done |= one
        m = ~done
        ixm = ix[m] + _U(0x3F800000 - 0x3F3504F3)
        km = k[m] + (ixm >> _U(23)).astype(np.int32) - 0x7F
        ixm = (ixm & _U(0x007FFFFF)) + _U(0x3F3504F3)
        f = ixm.view(F) - F(1.0)
        hfsq = F(0.5) * f * f
        s = f / (F(2.0) + f)
        z = s * s
        w = z * z
        t1 = w * (LG2 + w * LG4)
        t2 = z * (LG1 + w * LG3)
        r = t2 + t1
        hi = ((f - hfsq).view(_U) & _U(0xFFFFF000)).view(F)
        lo = f - hi - hfsq + s * (hfsq + r)
        dk = km.astype(F)
        out[m] = dk * LOG10_2LO + (lo + hi) * IVLN10LO + lo * IVLN10HI + hi * IVLN10HI + dk * LOG10_2HI
    return out


def rust_max(a: np.ndarray, b) -> np.ndarray:
    """f32::max(a, b): a NaN loses; of two equal values b."""
    b = np.broadcast_to(np.asarray(b, F), a.shape)
    with np.errstate(all="ignore"):
        out = np.where(a > b, a, b)
    out = np.where(np.isnan(b), a, out)
    return np.where(np.isnan(a), b, out).astype(F)


def clamp01(t: np.ndarray) -> np.ndarray:
    """f32::clamp(0.0, 1.0): `if t < 0 {0} else if t > 1 {1} else {t}` -- a NaN and a -0 stay."""
    with np.errstate(all="ignore"):
        return np.where(t < F(0.0), F(0.0), np.where(t > F(1.0), F(1.0), t)).astype(F)


def as_u8(v: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        w = np.where(np.isnan(v), F(0.0), v)
        return np.trunc(np.clip(w, F(0.0), F(255.0))).astype(np.uint8)


def magnitude_to_db(mag, max_mag, floor_db, log10=None) -> np.ndarray:
    """spectrogram.rs:96-102"""
    mag = np.asarray(mag, F)
    shape = mag.shape
    mag = mag.reshape(-1)
    max_mag, floor_db = F(max_mag), F(floor_db)
    with np.errstate(all="ignore"):
        floored = np.full(mag.shape, max_mag <= F(0.0)) | (mag <= F(0.0))
        db = F(20.0) * libm_log10f(mag / max_mag, log10)
        return np.where(floored, floor_db, rust_max(db, floor_db)).astype(F).reshape(shape)


def db_scale(mag, max_mag, dynamic_range, log10=None) -> np.ndarray:
    """spectrogram.rs:107-110"""
    mag = np.asarray(mag, F)
    shape = mag.shape
    mag = mag.reshape(-1)
    max_mag, dr = F(max_mag), F(dynamic_range)
    with np.errstate(all="ignore"):
        db = F(20.0) * libm_log10f(rust_max(mag / max_mag, F(1e-10)), log10)
        return clamp01((db + dr) / dr).reshape(shape)


def _lerp(a: int, b: int, local: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        return as_u8(F(a) + (F(b) - F(a)) * local)


def fire_segment(t: np.ndarray) -> np.ndarray:
    """The index of the first window [s, e] of FIRE_STOPS with t >= s && t <= e; 3 (the fallback) where there is none."""
    seg = np.full(t.shape, 3, np.int64)
    taken = np.zeros(t.shape, bool)
    with np.errstate(all="ignore"):
        for i in range(4):
            hit = ~taken & (t >= F(FIRE_STOPS[i][0])) & (t <= F(FIRE_STOPS[i + 1][0]))
            seg[hit] = i
            taken |= hit
    return seg


def rainbow_segment(t: np.ndarray) -> np.ndarray:
    """`while i + 1 < 6 && t > STOPS[i + 1].0 { i += 1 }`"""
    i = np.zeros(t.shape, np.int64)
    going = np.ones(t.shape, bool)
    with np.errstate(all="ignore"):
        for step in range(5):
            going &= t > F(RAINBOW_STOPS[step + 1][0])
            i[going] = step + 1
    return i


def map_color_u8(t, cmap: int) -> np.ndarray:
    """spectrogram.rs:113-187 on an array of t: [..., 3] uint8."""
    t = clamp01(np.asarray(t, F).reshape(-1))
    out = np.zeros((t.size, 3), np.uint8)
    with np.errstate(all="ignore"):
        if cmap == FIRE or cmap == RAINBOW:
            stops = FIRE_STOPS if cmap == FIRE else RAINBOW_STOPS
            seg = fire_segment(t) if cmap == FIRE else rainbow_segment(t)
            for i in range(len(stops) - 1):
                sel = seg == i
                j = min(i + 1, len(stops) - 1)
                (t0, c0), (t1, c1) = stops[i], stops[j]
                t0, t1 = F(t0), F(t1)
                local = (t[sel] - t0) / (t1 - t0)
                for ch in range(3):
                    out[sel, ch] = _lerp(c0[ch], c1[ch], local)
            assert cmap == FIRE or seg.max(initial=0) <= 4
        elif cmap == LEGACY:
            out[:, 0] = as_u8(F(64.0) * (F(1.0) - t) + F(255.0) * t)
            out[:, 1] = as_u8(F(255.0) * t)
            out[:, 2] = as_u8(F(64.0) * (F(1.0) - t) + F(224.0) * t)
        elif cmap == GRAY:
            v = t * F(255.0)
            r = np.trunc(v)
            r = np.where(v - r >= F(0.5), r + F(1.0), r)  # f32::round on [0, 255]: half away from zero
            out[:] = as_u8(r)[:, None]
        else:
            raise ValueError("the colorous palettes are not restated")
    return out


def map_color_u16(t, cmap: int) -> np.ndarray:
    return map_color_u8(t, cmap).astype(np.uint16) * np.uint16(257)


def color_t(mag, max_mag, mode: int, level, log10=None) -> np.ndarray:
    """The palette argument of every magnitude: mode 0 color_from_magnitude's (spectrogram.rs:196-199), mode 1 db_scale."""
    level = F(level)
    if mode == 1:
        return db_scale(mag, max_mag, level, log10)
    with np.errstate(all="ignore"):
        return ((magnitude_to_db(mag, max_mag, level, log10) - level) / -level).astype(F)


def map_bin_to_pixel(b: int, max_bin: int) -> int:
    """spectrogram.rs:209-217 with glibc's logf; the saturating cast."""
    if max_bin == 0:
        return 0
    log_max = F(_libm.logf(F(max_bin) + F(1.0)))
    pos = F(_libm.logf(F(b) + F(1.0)))
    with np.errstate(all="ignore"):
        v = np.floor(F(max_bin) * pos / log_max)
    if np.isnan(v) or v <= 0:
        return 0
    return int(min(float(v), float(2 ** 64 - 1)))


def log_bin_map(bins: int) -> np.ndarray:
    return np.array([min(map_bin_to_pixel(b, bins - 1), 2 ** 32 - 1) for b in range(bins)], np.uint32)


def log_scale_bins(frames: np.ndarray, table) -> np.ndarray:
    """spectrogram.rs:220-234 on every row of [frames, bins] with y = table[bin]: accum[y] += v in increasing bin order, then one
    division by the count."""
    x = np.asarray(frames, F)
    n, bins = x.shape
    accum = np.zeros((n, bins), F)
    counts = np.zeros(bins, np.uint32)
    with np.errstate(all="ignore"):
        for b in range(bins):
            y = int(table[b])
            accum[:, y] = accum[:, y] + x[:, b]
            counts[y] += 1
        live = counts > 0
        accum[:, live] = accum[:, live] / counts[live].astype(F)
    return accum


def render(mags, max_mag, mode: int, level, cmap: int, depth: int, scale: int, layout: int, table=None, log10=None) -> np.ndarray:
    """[frames, bins] -> [frames, bins, 3] (layout 0) or the picture [bins, frames, 3] with bin b at row bins - 1 - b (layout 1);
    uint8, or uint16 = the 8-bit value * 257."""
    x = np.asarray(mags, F)
    frames, bins = x.shape
    if scale == 1:
        x = log_scale_bins(x, log_bin_map(bins) if table is None else table)
    px = map_color_u8(color_t(x.reshape(-1), max_mag, mode, level, log10), cmap).reshape(frames, bins, 3)
    if depth == 16:
        px = px.astype(np.uint16) * np.uint16(257)
    if layout == 1:
        px = np.ascontiguousarray(px[:, ::-1, :].transpose(1, 0, 2))
    return np.ascontiguousarray(px)
