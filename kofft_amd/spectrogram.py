"""visual::spectrogram's colour helpers (visual/spectrogram.rs:96-234) on the device: ``magnitude_to_db``, ``db_scale``, and ``render``,
which turns the [frames, bins] magnitudes of ``stft_magnitudes`` into an RGB picture (``color_from_magnitude_u8 / _u16``, or
``map_color(db_scale(..))``, with optional ``log_scale_bins``), plus the host helpers ``log_bin_map`` (``map_bin_to_pixel`` for every
bin) and ``map_color_u8`` (a legend); and ``from_audio``, which goes from samples to pictures in one call (the row's, the running
or a given maximum) without the magnitudes ever leaving the context's scratch.

The arithmetic is the reference's f32 operation order bit for bit, with the **libm crate's** ``log10f`` where the reference calls
``.log10()`` (include/kofft_hip.h).  Fire, Legacy, Gray and Rainbow are implemented; Viridis, Plasma and Inferno (the
colorous crate's tables) raise FftError(InvalidValue).

A numpy array goes through the host-pointer call and gives a numpy array.  A torch tensor on the device goes through the
device-pointer call and gives a torch tensor on the device: the call is asynchronous on the context's stream (``fft.synchronize()``, or
``fft.set_stream`` with torch's stream), and with ``max_mag`` a device tensor too -- the ``d_max`` of ``stft_magnitudes_rows_dev`` --
nothing travels to the host.  ``fft=`` is the f32 HipFftImpl to run on; without one, a context on device 0 is created at the first
call and kept."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from .api import DeviceError, FftError, HipFftImpl, _direct_ctx, _ptr

__all__ = ["COLORMAPS", "FIRE", "LEGACY", "GRAY", "VIRIDIS", "PLASMA", "INFERNO", "RAINBOW", "db_scale", "from_audio", "log_bin_map",
           "magnitude_to_db", "map_color_u8", "render", "set_transpose"]

FIRE, LEGACY, GRAY, VIRIDIS, PLASMA, INFERNO, RAINBOW = range(7)  # Colormap's declaration order (spectrogram.rs:16-31)
COLORMAPS = {"fire": FIRE, "legacy": LEGACY, "gray": GRAY, "viridis": VIRIDIS, "plasma": PLASMA, "inferno": INFERNO, "rainbow": RAINBOW}
_SCALES = {"linear": 0, "log": 1}
_LAYOUTS = {"frames": 0, "image": 1}
_MAX_MODES = {"row": 0, "running": 1, "given": 2}


def _enum(value, names, what) -> int:
    if isinstance(value, str):
        if value.lower() not in names:
            raise ValueError(f"unknown {what} {value!r}: one of {sorted(names)}")
        return names[value.lower()]
    return int(value)


def _raise(rc: int, what: str):
    if rc > 0:
        raise FftError(rc)
    if rc < 0:
        raise DeviceError(rc, what)


def log_bin_map(bins: int) -> np.ndarray:
    """map_bin_to_pixel(b, bins - 1) (spectrogram.rs:209-217) for every b < bins: a uint32 array, computed in f32 with glibc's logf."""
    if int(bins) < 0:
        raise ValueError("bins is a usize in the reference: it cannot be negative")
    out = np.empty(int(bins), np.uint32)
    _raise(_lib.load().kofft_hip_log_bin_map(int(bins), _ptr(out)), "log_bin_map takes bins <= 2^24")
    return out


def map_color_u8(t: float, cmap="fire") -> np.ndarray:
    """map_color_u8 (spectrogram.rs:113-160) on the host: three uint8 values."""
    out = np.zeros(3, np.uint8)
    _raise(_lib.load().kofft_hip_map_color_u8(float(t), _enum(cmap, COLORMAPS, "colormap"), _ptr(out)), "map_color_u8")
    return out


def set_transpose(on: bool, fft: Optional[HipFftImpl] = None) -> None:
    """True (the default): the image layout leaves through an LDS tile, whole dwords per picture row; False: every lane stores its own
    bytes -- the same bytes, for A/B measurements and tests."""
    f = _direct_ctx(fft)
    f._check(f._lib.kofft_hip_set_spectrogram_transpose(f._ctx, int(bool(on))))


def _is_dev(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def _inputs(mags, max_mag, what):
    """-> (magnitudes, max_mag as one float32 where the magnitudes live, is a device tensor)"""
    if _is_dev(mags):
        import torch

        if not mags.is_cuda or mags.dtype != torch.float32:
            raise TypeError(f"{what}: a torch input must be a float32 tensor on the device")
        a = mags.contiguous()
        if _is_dev(max_mag):
            if not max_mag.is_cuda or max_mag.dtype != torch.float32 or max_mag.numel() != 1:
                raise TypeError(f"{what}: a torch max_mag must be one float32 on the device")
            m = max_mag.contiguous()
        else:
            m = torch.tensor([float(max_mag)], dtype=torch.float32, device=a.device)
        return a, m, True
    if _is_dev(max_mag):
        raise TypeError(f"{what}: a device max_mag needs device magnitudes")
    return np.ascontiguousarray(mags, np.float32), np.array([max_mag], np.float32).reshape(1), False


def _pointwise(stem, mags, max_mag, level, fft):
    a, m, dev = _inputs(mags, max_mag, stem)
    f = _direct_ctx(fft)
    if dev:
        import torch

        out = torch.empty_like(a)
        f._check(getattr(f._lib, f"kofft_hip_dev_{stem}_f32")(f._ctx, C.c_void_p(a.data_ptr()), a.numel(), C.c_void_p(m.data_ptr()), float(level),
                                                            C.c_void_p(out.data_ptr())))
    else:
        out = np.empty_like(a)
        f._check(getattr(f._lib, f"kofft_hip_{stem}_f32")(f._ctx, _ptr(a), a.size, _ptr(m), float(level), _ptr(out)))
    return out


def magnitude_to_db(mags, max_mag, floor_db: float, fft: Optional[HipFftImpl] = None):
    """magnitude_to_db (spectrogram.rs:96-102) of every value: float32, the input's shape.  An empty input raises FftError(EmptyInput)."""
    return _pointwise("magnitude_to_db", mags, max_mag, floor_db, fft)


def db_scale(mags, max_mag, dynamic_range: float, fft: Optional[HipFftImpl] = None):
    """db_scale (spectrogram.rs:107-110) of every value: float32 in [0, 1], the input's shape."""
    return _pointwise("db_scale", mags, max_mag, dynamic_range, fft)


def render(mags, max_mag, mode: int = 0, level: float = -120.0, cmap="fire", depth: int = 8, scale="linear", layout="image",
           pix_of_bin=None, fft: Optional[HipFftImpl] = None):
    """[frames, bins] magnitudes -> an RGB picture.  mode 0: color_from_magnitude with `level` the floor in dB; mode 1:
    map_color(db_scale(..)) with `level` the dynamic range.  depth 8: uint8; 16: uint16, the 8-bit value * 257.  scale "log": every
    frame through log_scale_bins(frame, bins - 1) first, over `pix_of_bin` (default: log_bin_map(bins)).  layout "image":
    [bins, frames, 3] with bin b at row bins - 1 - b (low frequencies at the bottom); "frames": [frames, bins, 3]."""
    a, m, dev = _inputs(mags, max_mag, "render")
    if a.ndim != 2:
        raise TypeError("render expects 2-D [frames, bins] magnitudes")
    frames, bins = int(a.shape[0]), int(a.shape[1])
    cmap, scale, layout = _enum(cmap, COLORMAPS, "colormap"), _enum(scale, _SCALES, "scale"), _enum(layout, _LAYOUTS, "layout")
    if frames == 0 or bins == 0:
        raise FftError(FftError.EmptyInput)
    if int(depth) not in (8, 16):
        raise FftError(FftError.InvalidValue)
    table = None
    if scale == 1:
        table = log_bin_map(bins) if pix_of_bin is None else np.ascontiguousarray(pix_of_bin, np.uint32)
        if table.ndim != 1 or table.size != bins:
            raise FftError(FftError.MismatchedLengths)
    shape = (frames, bins, 3) if layout == 0 else (bins, frames, 3)
    f = _direct_ctx(fft)
    args = (frames, bins, None, int(mode), float(level), cmap, int(depth), scale, layout, _ptr(table))
    if dev:
        import torch

        dt = torch.uint8 if int(depth) == 8 else getattr(torch, "uint16", torch.int16)
        out = torch.empty(shape, dtype=dt, device=a.device)
        f._check(f._lib.kofft_hip_dev_spectrogram_render_f32(f._ctx, C.c_void_p(a.data_ptr()), frames, bins, C.c_void_p(m.data_ptr()), *args[3:],
                                                             C.c_void_p(out.data_ptr())))
    else:
        out = np.empty(shape, np.uint8 if int(depth) == 8 else np.uint16)
        f._check(f._lib.kofft_hip_spectrogram_render_f32(f._ctx, _ptr(a), frames, bins, _ptr(m), *args[3:], _ptr(out)))
    return out


def from_audio(signals, win_len: int, hop: int, *, window=None, frames: Optional[int] = None, max_mode="row", max_mag=None, mode: int = 0,
               level: float = -120.0, cmap="fire", depth: int = 8, channels: int = 3, scale="linear", layout="image", pix_of_bin=None,
               fft: Optional[HipFftImpl] = None, return_max: bool = False):
    """Audio -> spectrogram pictures in one call (kofft_hip_stft_picture_f32): what examples/spectrogram.rs and
    sanity-check do with ``stft_magnitudes``, its maximum and ``color_from_magnitude_u8`` (max_mode "row"), and what web-spectrogram's
    ``compute_frame`` does a frame at a time with its running maximum from 1e-12 (max_mode "running"; layout "frames" with channels 4
    gives its RGBA rows); "given" colours against ``max_mag``, one value per row.  The magnitudes stay in the context's scratch.

    A 1-D signal gives one picture, a 2-D [rows, len] array one per row: [(rows,) bins, frames, channels] for layout "image",
    [(rows,) frames, bins, channels] for "frames", bins = win_len // 2; uint8, or uint16 at depth 16 (channels 3 only).  ``window``
    None is window::hann(win_len); ``frames`` defaults to ceil(len / hop).  The other arguments are ``render``'s.  numpy in, numpy out
    through the host-pointer call; a float32 torch tensor on the device goes through the device-pointer call (asynchronous on the
    context's stream) and gives torch tensors, ``window`` and ``max_mag`` being device tensors then (or None).  return_max=True:
    (pictures, the maximum used: per row, float32)."""
    max_mode = _enum(max_mode, _MAX_MODES, "max_mode")
    cmap, scale, layout = _enum(cmap, COLORMAPS, "colormap"), _enum(scale, _SCALES, "scale"), _enum(layout, _LAYOUTS, "layout")
    if max_mode not in (0, 1, 2) or layout not in (0, 1) or scale not in (0, 1) or int(depth) not in (8, 16) or int(channels) not in (3, 4):
        raise FftError(FftError.InvalidValue)
    if (int(channels) == 4 and int(depth) == 16) or (max_mode == 1 and scale == 1):
        raise FftError(FftError.InvalidValue)
    if int(hop) == 0:
        raise FftError(FftError.InvalidHopSize)
    if int(win_len) < 0 or int(hop) < 0:
        raise ValueError("win_len and hop are usize in the reference: they cannot be negative")
    if max_mode == 2 and max_mag is None:
        raise TypeError('max_mode "given" needs max_mag, one float32 per row')
    bins = int(win_len) // 2
    table = None
    if scale == 1:
        table = log_bin_map(bins) if pix_of_bin is None else np.ascontiguousarray(pix_of_bin, np.uint32)
        if table.ndim != 1 or table.size != bins:
            raise FftError(FftError.MismatchedLengths)
    if not _is_dev(signals):
        signals = np.asarray(signals, np.float32)
    if signals.ndim not in (1, 2):
        raise TypeError("from_audio expects a 1-D signal or a 2-D [rows, len] array")
    one = signals.ndim == 1
    need = -(-int(signals.shape[-1]) // int(hop))
    nf = need if frames is None else int(frames)
    if nf < need:
        raise FftError(FftError.MismatchedLengths)
    if window is not None and int(window.numel() if _is_dev(window) else np.size(window)) != int(win_len):
        raise TypeError("window must hold win_len values")
    f = _direct_ctx(fft)
    if not _is_dev(signals):
        sig = np.ascontiguousarray(signals, np.float32).reshape(1 if one else signals.shape[0], -1)
        mx = None if max_mode != 2 else np.broadcast_to(np.asarray(max_mag, np.float32).reshape(-1), (sig.shape[0],))
        out, used = f.stft_picture_rows(sig, win_len, hop, window, nf, max_mode, mx, mode, level, cmap, depth, channels, scale, layout, table)
    else:
        import torch

        if not signals.is_cuda or signals.dtype != torch.float32:
            raise TypeError("from_audio: a torch input must be a float32 tensor on the device")
        sig = signals.contiguous().reshape(1 if one else signals.shape[0], -1)
        rows, length = int(sig.shape[0]), int(sig.shape[1])
        for name, t, n in (("window", window, int(win_len)), ("max_mag", max_mag if max_mode == 2 else None, rows)):
            if t is not None and not (_is_dev(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n):
                raise TypeError(f"from_audio: a device signal takes {name} as a contiguous float32 device tensor of {n} values")
        dt = torch.uint8 if int(depth) == 8 else getattr(torch, "uint16", torch.int16)
        shape = (rows, nf, bins, int(channels)) if layout == 0 else (rows, bins, nf, int(channels))
        out = torch.zeros(shape, dtype=dt, device=sig.device)
        used = torch.zeros(rows, dtype=torch.float32, device=sig.device)
        f.stft_picture_rows_dev(sig.data_ptr() if length else 0, rows, length, length, 0 if window is None else window.data_ptr(), win_len, hop, nf,
                                max_mode, max_mag.data_ptr() if max_mode == 2 else 0, used.data_ptr(), mode, level, cmap, depth, channels, scale,
                                layout, table, out.data_ptr())
    if one:
        out, used = out[0], used[0]
    return (out, used) if return_max else out
