"""kofft::goertzel (goertzel.rs) -- the single-bin detector with the reference's name, on the device.

goertzel_f32(input, sample_rate, target_freq) is the reference's call: one magnitude, bit for bit (include/kofft_hip.h).  The batched
extension takes a 2-D [batch, n] input and a sequence of frequencies and gives [batch, nfreq].
"""
from typing import Optional

import numpy as np

from . import api

__all__ = ["goertzel_f32"]


def _empty(input, shape):
    """An empty float32 result of the input's kind: a torch tensor on its device for a tensor, a numpy array otherwise."""
    if hasattr(input, "data_ptr") and hasattr(input, "is_cuda"):
        import torch

        return torch.empty(shape, dtype=torch.float32, device=input.device)
    return np.empty(shape, np.float32)


def goertzel_f32(input, sample_rate: float, target_freq, fft: Optional[api.HipFftImpl] = None):
    """goertzel.rs:16-36.  A 1-D signal and a scalar frequency: a Python float.  A 2-D [batch, n] input and / or a sequence of
    frequencies: a float32 array [batch, nfreq] (or [nfreq] for a 1-D signal).  FftError(EmptyInput) for an empty signal, then
    FftError(InvalidValue) for sample_rate <= 0, as in the reference."""
    shape = tuple(input.shape) if hasattr(input, "shape") else np.shape(input)
    if len(shape) not in (1, 2):
        raise TypeError("goertzel_f32 expects a 1-D signal or a 2-D [batch, n] array")
    scalar = np.ndim(target_freq) == 0
    nfreq = 1 if scalar else int(np.size(target_freq))
    if len(shape) == 2 and shape[0] == 0:
        return _empty(input, (0, nfreq))
    api.goertzel_check(shape[-1], sample_rate, nfreq)
    if nfreq == 0:
        return _empty(input, shape[:-1] + (0,))
    out = api._direct_ctx(fft).goertzel(input, sample_rate, target_freq)
    if scalar and len(shape) == 1:
        return float(out[0])
    return out
