"""kofft::dct (dct.rs:108-305): the direct DCT-I .. DCT-IV of f32 signals on the device, the reference's naive sums bit for bit.

``dct1`` .. ``dct4`` take a 1-D signal or a 2-D [batch, n] array and return a new float32 array; ``batch_i`` .. ``batch_iv`` and
``multi_channel_i`` .. ``multi_channel_iv`` transform a list of 1-D float32 rows of any lengths in place, one device call per
length.  ``fft=`` names the f32 HipFftImpl to run on; without one, a context on device 0 is created at the first call and kept.
Errors are raised before any device is touched: n == 0 gives an empty result, except for dct3 (FftError(EmptyInput): the reference
indexes input[0] unchecked); n > 4096 raises DeviceError (the bound of the library's table).  ``dct2`` here is dct::dct2, not
``DctPlanner.plan_dct2`` (FFT-based, another rounding)."""
from __future__ import annotations

from typing import Optional

from .api import HipFftImpl, direct_batch_inplace, direct_transform

__all__ = ["dct1", "dct2", "dct3", "dct4", "batch_i", "batch_ii", "batch_iii", "batch_iv",
           "multi_channel_i", "multi_channel_ii", "multi_channel_iii", "multi_channel_iv"]


def dct1(input, fft: Optional[HipFftImpl] = None):
    """dct::dct1 (dct.rs:108-131)."""
    return direct_transform("dct", 1, input, fft)


def dct2(input, fft: Optional[HipFftImpl] = None):
    """dct::dct2 (dct.rs:134-146)."""
    return direct_transform("dct", 2, input, fft)


def dct3(input, fft: Optional[HipFftImpl] = None):
    """dct::dct3 (dct.rs:149-161)."""
    return direct_transform("dct", 3, input, fft)


def dct4(input, fft: Optional[HipFftImpl] = None):
    """dct::dct4 (dct.rs:164-176)."""
    return direct_transform("dct", 4, input, fft)


def batch_i(batches, fft: Optional[HipFftImpl] = None) -> None:
    """dct::batch_i (dct.rs:263-268): every row replaced by its dct1."""
    direct_batch_inplace("dct", 1, batches, fft)


def batch_ii(batches, fft: Optional[HipFftImpl] = None) -> None:
    """dct::batch_ii (dct.rs:270-275)."""
    direct_batch_inplace("dct", 2, batches, fft)


def batch_iii(batches, fft: Optional[HipFftImpl] = None) -> None:
    """dct::batch_iii (dct.rs:277-282)."""
    direct_batch_inplace("dct", 3, batches, fft)


def batch_iv(batches, fft: Optional[HipFftImpl] = None) -> None:
    """dct::batch_iv (dct.rs:284-289)."""
    direct_batch_inplace("dct", 4, batches, fft)


def multi_channel_i(channels, fft: Optional[HipFftImpl] = None) -> None:
    """dct::multi_channel_i (dct.rs:291-293): batch_i."""
    batch_i(channels, fft)


def multi_channel_ii(channels, fft: Optional[HipFftImpl] = None) -> None:
    """dct::multi_channel_ii (dct.rs:295-297): batch_ii."""
    batch_ii(channels, fft)


def multi_channel_iii(channels, fft: Optional[HipFftImpl] = None) -> None:
    """dct::multi_channel_iii (dct.rs:299-301): batch_iii."""
    batch_iii(channels, fft)


def multi_channel_iv(channels, fft: Optional[HipFftImpl] = None) -> None:
    """dct::multi_channel_iv (dct.rs:303-305): batch_iv."""
    batch_iv(channels, fft)
