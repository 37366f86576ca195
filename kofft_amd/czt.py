"""kofft::czt (czt.rs) -- the chirp-Z transform with the reference's name, on the device.

czt_f32(input, m, w, a) evaluates sum_i x[i] * a^-i * w^(i k) at k = 0 .. m - 1 with the reference's f32 recurrences, bit for bit
(include/kofft_hip.h).  A 2-D [batch, n] input transforms every row in one call.
"""
from typing import Optional

import numpy as np

from . import api

__all__ = ["czt_f32"]


def _empty(input, shape):
    """An empty complex64 result of the input's kind: a torch tensor on its device for a tensor, a numpy array otherwise."""
    if hasattr(input, "data_ptr") and hasattr(input, "is_cuda"):
        import torch

        return torch.empty(shape, dtype=torch.complex64, device=input.device)
    return np.empty(shape, np.complex64)


def czt_f32(input, m: int, w, a, fft: Optional[api.HipFftImpl] = None):
    """czt.rs:16-54: [m] complex64 for a 1-D signal, [batch, m] for a 2-D [batch, n] array (numpy in, numpy out; a torch tensor on the
    device stays there).  w and a are complex numbers or (re, im) pairs.  m == 0 gives an empty result; an empty signal m zeros."""
    shape = tuple(input.shape) if hasattr(input, "shape") else np.shape(input)
    if len(shape) not in (1, 2):
        raise TypeError("czt_f32 expects a 1-D signal or a 2-D [batch, n] array")
    if not api.czt_check(shape[-1], int(m)):
        return _empty(input, shape[:-1] + (0,))
    if len(shape) == 2 and shape[0] == 0:
        return _empty(input, (0, int(m)))
    return api._direct_ctx(fft).czt(input, int(m), w, a)
