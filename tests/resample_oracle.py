"""The polyphase resampler's definition (include/kofft_hip.h) in numpy float32: output m of a row sits at up-sampled
time t = t0 + m * down, p = t mod up, i0 = t div up, and is the sum over ascending j (while p + j * up < nh) of h[p + j * up] * x[i0 - j]
in one f32 accumulator seeded with +0, product and sum separate f32 operations, the terms with i0 - j outside [0, nx) skipped.
Vectorised over rows and outputs, one j at a time, so the order of every output's additions is the definition's.  Positions are int64."""
from __future__ import annotations

import numpy as np

F = np.float32


def positions(up, down, t0, out_len):
    """(p, i0) of outputs 0 .. out_len - 1, int64."""
    t = np.int64(t0) + np.arange(out_len, dtype=np.int64) * np.int64(down)
    return t % np.int64(up), t // np.int64(up)


def resample_ref(x, h, up, down, t0, out_len, x_first=0, nx=None):
    """[rows, out_len] float32 for x [rows, n] (or 1-D: one row) and taps h [nh].  x_first / nx: x holds samples x_first .. x_first + n - 1
    of rows of nx samples (a window near the end of a long row); every term of the requested outputs must lie inside it or outside
    the row."""
    x = np.ascontiguousarray(x, F)
    h = np.ascontiguousarray(h, F)
    x2 = x.reshape(-1, x.shape[-1])
    n = x2.shape[1]
    nx = x_first + n if nx is None else nx
    nh = h.shape[0]
    p, i0 = positions(up, down, t0, out_len)
    acc = np.zeros((x2.shape[0], out_len), F)
    for j in range((nh - 1) // up + 1):
        k = p + j * up
        i = i0 - j
        live = (k < nh) & (i >= 0) & (i < nx)
        if not live.any():
            continue
        assert (i[live] >= x_first).all() and (i[live] < x_first + n).all(), "a term outside the samples given"
        prod = h[k[live]][None, :] * x2[:, i[live] - x_first]  # one f32 product
        acc[:, live] = acc[:, live] + prod                     # one f32 sum
    return acc.reshape(x.shape[:-1] + (out_len,))


def term_stats(x, h, up, down, t0, out_len):
    """Per output of a 1-D x: (J, sum |h_k x_i|) over its live terms, in float64: the CPU tests' forward error bound."""
    x = np.asarray(x, np.float64)
    h = np.asarray(h, np.float64)
    nx, nh = x.shape[0], h.shape[0]
    p, i0 = positions(up, down, t0, out_len)
    count = np.zeros(out_len, np.int64)
    mag = np.zeros(out_len, np.float64)
    for j in range((nh - 1) // up + 1):
        k = p + j * up
        i = i0 - j
        live = (k < nh) & (i >= 0) & (i < nx)
        count[live] += 1
        mag[live] += np.abs(h[k[live]] * x[i[live]])
    return count, mag


def forward_bound(x, h, up, down, t0, out_len):
    """(J + 2) u sum |h_k x_i| per output of a 1-D x, u = 2^-24: the forward error of recursive summation of J rounded products
    (Higham, Accuracy and Stability of Numerical Algorithms, 4.2: (J - 1) u for the sums and u for the products to first order), with
    two units to spare for the higher-order terms.  Nothing measured."""
    count, mag = term_stats(x, h, up, down, t0, out_len)
    return (count + 2) * 2.0 ** -24 * mag


def full_len(nx, nh, up, down):
    """scipy.signal.upfirdn's output length: ceil(((nx - 1) * up + nh) / down)."""
    return -(-((nx - 1) * up + nh) // down)
