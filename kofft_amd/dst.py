"""kofft::dst (dst.rs:18-191): the direct DST-I .. DST-IV of f32 signals on the device, the reference's naive sums bit for bit, and
the DstPlanner's sine tables.

``dst1`` .. ``dst4`` take a 1-D signal or a 2-D [batch, n] array and return a new float32 array; ``batch_i`` .. ``batch_iv`` and
``multi_channel_i`` .. ``multi_channel_iv`` transform a list of 1-D float32 rows of any lengths in place, one device call per
length.  ``fft=`` names the f32 HipFftImpl to run on; without one, a context on device 0 is created at the first call and kept.
Errors are raised before any device is touched: n == 0 gives an empty result, except for dst3 (FftError(EmptyInput): the reference
indexes input[0] unchecked); n > 4096 raises DeviceError (the bound of the library's table)."""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _lib
from .api import HipFftImpl, _ptr, direct_batch_inplace, direct_transform

__all__ = ["DstPlanner", "dst1", "dst2", "dst3", "dst4", "batch_i", "batch_ii", "batch_iii", "batch_iv",
           "multi_channel_i", "multi_channel_ii", "multi_channel_iii", "multi_channel_iv"]


class DstPlanner:
    """DstPlanner<T> (dst.rs:18-86): sin(factor * (i + off)) tables, factor = pi / n, cached per length; built by the library's
    host recipe (glibc sinf for float32, sin for float64)."""

    def __init__(self, dtype=np.float32):
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise TypeError("DstPlanner is f32 or f64")
        self._caches: dict[int, dict[int, np.ndarray]] = {2: {}, 3: {}, 4: {}}
        self._scratch = np.zeros(0, self.dtype)

    def _plan(self, type: int, n: int) -> np.ndarray:
        n = int(n)
        cache = self._caches[type]
        if n not in cache:
            t = np.empty(n, self.dtype)
            fn = _lib.load().kofft_hip_dst_planner_table_f32 if self.dtype == np.float32 else _lib.load().kofft_hip_dst_planner_table_f64
            rc = fn(type, n, _ptr(t))
            if rc:
                raise RuntimeError(f"kofft_hip_dst_planner_table: status {rc}")
            t.flags.writeable = False
            cache[n] = t
        return cache[n]

    def plan_dst2(self, n: int) -> np.ndarray:
        """dst.rs:53-59: offset 0.5."""
        return self._plan(2, n)

    def plan_dst3(self, n: int) -> np.ndarray:
        """dst.rs:62-68: offset 0.0."""
        return self._plan(3, n)

    def plan_dst4(self, n: int) -> np.ndarray:
        """dst.rs:71-77: offset 0.5."""
        return self._plan(4, n)

    def scratch(self, len: int) -> np.ndarray:
        """dst.rs:80-85: a view of at least ``len`` elements of the planner's reusable buffer (grown with zeros)."""
        len = int(len)
        if self._scratch.shape[0] < len:
            grown = np.zeros(len, self.dtype)
            grown[: self._scratch.shape[0]] = self._scratch
            self._scratch = grown
        return self._scratch[:len]


def dst1(input, fft: Optional[HipFftImpl] = None):
    """dst::dst1 (dst.rs:89-101)."""
    return direct_transform("dst", 1, input, fft)


def dst2(input, fft: Optional[HipFftImpl] = None):
    """dst::dst2 (dst.rs:104-116)."""
    return direct_transform("dst", 2, input, fft)


def dst3(input, fft: Optional[HipFftImpl] = None):
    """dst::dst3 (dst.rs:119-131)."""
    return direct_transform("dst", 3, input, fft)


def dst4(input, fft: Optional[HipFftImpl] = None):
    """dst::dst4 (dst.rs:134-146)."""
    return direct_transform("dst", 4, input, fft)


def batch_i(batches, fft: Optional[HipFftImpl] = None) -> None:
    """dst::batch_i (dst.rs:149-154): every row replaced by its dst1."""
    direct_batch_inplace("dst", 1, batches, fft)


def batch_ii(batches, fft: Optional[HipFftImpl] = None) -> None:
    """dst::batch_ii (dst.rs:156-161)."""
    direct_batch_inplace("dst", 2, batches, fft)


def batch_iii(batches, fft: Optional[HipFftImpl] = None) -> None:
    """dst::batch_iii (dst.rs:163-168)."""
    direct_batch_inplace("dst", 3, batches, fft)


def batch_iv(batches, fft: Optional[HipFftImpl] = None) -> None:
    """dst::batch_iv (dst.rs:170-175)."""
    direct_batch_inplace("dst", 4, batches, fft)


def multi_channel_i(channels, fft: Optional[HipFftImpl] = None) -> None:
    """dst::multi_channel_i (dst.rs:177-179): batch_i."""
    batch_i(channels, fft)


def multi_channel_ii(channels, fft: Optional[HipFftImpl] = None) -> None:
    """dst::multi_channel_ii (dst.rs:181-183): batch_ii."""
    batch_ii(channels, fft)


def multi_channel_iii(channels, fft: Optional[HipFftImpl] = None) -> None:
    """dst::multi_channel_iii (dst.rs:185-187): batch_iii."""
    batch_iii(channels, fft)


def multi_channel_iv(channels, fft: Optional[HipFftImpl] = None) -> None:
    """dst::multi_channel_iv (dst.rs:189-191): batch_iv."""
    batch_iv(channels, fft)
