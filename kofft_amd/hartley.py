"""kofft::hartley (hartley.rs:12-57): the discrete Hartley transform of f32 signals on the device, the reference's naive sums bit for
bit -- the libm crate's cosf / sinf in the table, one f32 multiply and one f32 add per term.

``dht`` takes a 1-D signal or a 2-D [batch, n] array and returns a new float32 array; ``batch`` and ``multi_channel`` transform a list
of 1-D float32 rows of any lengths in place, one device call per length.  ``fft=`` names the f32 HipFftImpl to run on; without one, a
context on device 0 is created at the first call and kept.  Errors are raised before any device is touched: n == 0 gives an empty
result; n > 4096 raises DeviceError (the bound of the library's table)."""
from __future__ import annotations

from typing import Optional

from .api import HipFftImpl, dht_batch_inplace, dht_transform

__all__ = ["dht", "batch", "multi_channel"]


def dht(input, fft: Optional[HipFftImpl] = None):
    """hartley::dht (hartley.rs:12-27)."""
    return dht_transform(input, fft)


def batch(batches, fft: Optional[HipFftImpl] = None) -> None:
    """hartley::batch (hartley.rs:48-53): every row replaced by its dht."""
    dht_batch_inplace(batches, fft)


def multi_channel(channels, fft: Optional[HipFftImpl] = None) -> None:
    """hartley::multi_channel (hartley.rs:55-57): batch."""
    batch(channels, fft)
