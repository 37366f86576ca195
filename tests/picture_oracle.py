"""Expected values of the audio -> spectrogram pictures call (kofft_hip_stft_picture_f32): the existing oracles composed.  The
magnitudes are tests/frontend_oracle.py's; the row maximum is stft_magnitudes' `if mag > max` scan from +0 over the flat row; the
running maximum is web-spectrogram's compute_frame (m from 1e-12, `if mag > m { m = mag }` walking frames then bins, BEFORE the pixel
is coloured) as np.maximum.accumulate over the row with every NaN replaced by the seed; the colours are tests/spectrogram_oracle.py's,
with an elementwise-maximum variant of its two dB functions for the running maximum.  `compute_frame_literal` restates compute_frame
as the scalar loop it is, for the test that pins the accumulate form against it.  Test infrastructure: nothing here calls the library."""
from __future__ import annotations

import numpy as np

import frontend_oracle as fo
import spectrogram_oracle as so

F = np.float32
SEED = F(1e-12)


def row_max(mags: np.ndarray) -> np.float32:
    """spectrogram.rs:65-73 over one row's [frames, bins]: from +0, `if mag > max`; a NaN is never selected."""
    m = np.asarray(mags, F).reshape(-1)
    m = m[~np.isnan(m)]
    return F(max(F(0.0), m.max(initial=F(0.0))))


def running_max(mags: np.ndarray) -> np.ndarray:
    """[frames, bins] -> the m every pixel is coloured with: the maximum of {1e-12} and the non-NaN magnitudes up to and including it."""
    m = np.asarray(mags, F)
    flat = np.where(np.isnan(m), SEED, m).reshape(-1)
    return np.maximum(np.maximum.accumulate(flat), SEED).astype(F).reshape(m.shape)


def compute_frame_literal(mags: np.ndarray):
    """web-spectrogram/src/lib.rs:211-234, its maximum only, as the scalar loop it is: ([frames, bins] m per pixel, the final m)."""
    m = np.asarray(mags, F)
    out = np.zeros(m.shape, F)
    mx = F(1e-12)
    for f in range(m.shape[0]):
        for o in range(m.shape[1]):
            mag = m[f, o]
            if mag > mx:  # (False for a NaN)
                mx = mag
            out[f, o] = mx
    return out, mx


def _db_elem(mag, mx, floor_db):
    """so.magnitude_to_db with one maximum per value"""
    floor_db = F(floor_db)
    with np.errstate(all="ignore"):
        floored = (mx <= F(0.0)) | (mag <= F(0.0))
        db = F(20.0) * so.libm_log10f(mag / mx)
        return np.where(floored, floor_db, so.rust_max(db, floor_db)).astype(F)


def _scale_elem(mag, mx, dynamic_range):
    """so.db_scale with one maximum per value"""
    dr = F(dynamic_range)
    with np.errstate(all="ignore"):
        db = F(20.0) * so.libm_log10f(so.rust_max(mag / mx, F(1e-10)))
        return so.clamp01((db + dr) / dr)


def render_elem(mags, mx, mode: int, level, cmap: int, depth: int, layout: int) -> np.ndarray:
    """so.render (linear scale) with a maximum per pixel: mx has mags' shape."""
    x = np.asarray(mags, F)
    frames, bins = x.shape
    v, m = x.reshape(-1), np.asarray(mx, F).reshape(-1)
    level = F(level)
    with np.errstate(all="ignore"):
        t = _scale_elem(v, m, level) if mode == 1 else ((_db_elem(v, m, level) - level) / -level).astype(F)
    px = so.map_color_u8(t, cmap).reshape(frames, bins, 3)
    if depth == 16:
        px = px.astype(np.uint16) * np.uint16(257)
    if layout == 1:
        px = np.ascontiguousarray(px[:, ::-1, :].transpose(1, 0, 2))
    return np.ascontiguousarray(px)


def with_alpha(px: np.ndarray, channels: int) -> np.ndarray:
    if channels == 3:
        return px
    out = np.full(px.shape[:-1] + (4,), 255, px.dtype)
    out[..., :3] = px
    return out


def pictures(mags: np.ndarray, max_mode: int, max_in=None, mode: int = 0, level=-120.0, cmap: int = 0, depth: int = 8, channels: int = 3,
             scale: int = 0, layout: int = 1, table=None):
    """[rows, frames, bins] magnitudes -> (pictures [rows, ...], max_out [rows])."""
    rows = mags.shape[0]
    out, mx = [], np.zeros(rows, F)
    for r in range(rows):
        if max_mode == 1:
            pm = running_max(mags[r])
            mx[r] = pm.reshape(-1)[-1] if pm.size else SEED
            px = render_elem(mags[r], pm, mode, level, cmap, depth, layout)
        else:
            mx[r] = row_max(mags[r]) if max_mode == 0 else F(max_in[r])
            px = so.render(mags[r], mx[r], mode, level, cmap, depth, scale, layout, table)
        out.append(with_alpha(px, channels))
    return np.stack(out), mx


def expected(oracle, x: np.ndarray, win_len: int, hop: int, frames: int, window=None, **kw):
    """Rows of samples -> (pictures, max_out, magnitudes)."""
    mags = fo.magnitudes(oracle, x, win_len, hop, frames, window)
    px, mx = pictures(mags, **kw)
    return px, mx, mags
