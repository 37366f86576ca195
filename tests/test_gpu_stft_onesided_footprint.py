"""The one-sided STFT entry points inside guard bands (tests/redzone.py), as tests/test_gpu_stft_rows_footprint.py does for the rows
family: every device-pointer form with its pointers in one arena on the device, every host-pointer form in a numpy arena through raw
ctypes calls.  A call writes its outputs and nothing else and leaves its `const` inputs alone.  For the forward call the rows of K bins
are written exactly: a store that should have been dropped and landed one row on shows as a wrong bin against the oracle, a store past
the last row shows in the band."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits_equal, seeded
from onesided_ref import bins, complete
from redzone import Arena

pytestmark = pytest.mark.gpu

# (win_len, hop, rows, frames, gap): the small kernels, the generic kernel with a tile-aligned and a ragged frame count, persistent group
# kernels (rows x frames past the threshold), one wavefront and several per transform, the composed route
SHAPES = [(1, 1, 5, 7, 3), (2, 1, 5, 7, 5), (16, 4, 5, 7, 5), (64, 16, 3, 16, 0), (256, 64, 7, 5, 3), (256, 64, 2731, 12, 5),
          (1024, 256, 3, 5, 5), (1024, 256, 1639, 5, 0), (4096, 1024, 3, 3, 1), (4096, 1024, 342, 3, 0), (400, 160, 5, 6, 5),
          (15, 4, 5, 6, 3)]


def _ids(s):
    return "win%d-hop%d-rows%d-frames%d-gap%d" % s


def _vp(r):
    return C.c_void_p(int(r))


@pytest.mark.parametrize("where", ["cuda", "host"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_stft_onesided_footprint(fft32, oracle, where, shape):
    win_len, hop, rows, frames, gap = shape
    length = max(1, frames * hop - 1)
    frames = -(-length // hop)
    stride = length + gap
    rng = seeded(68000 + win_len + rows)
    x = rng.uniform(-1, 1, (rows, length)).astype(np.float32)
    host = np.full((rows, stride), np.nan, np.float32)
    host[:, :length] = x
    flat = host.reshape(-1)[:(rows - 1) * stride + length]
    win = rng.uniform(0.1, 1, win_len).astype(np.float32)
    k = bins(win_len)
    lib, ctx, pre = fft32._lib, fft32._ctx, "kofft_hip_dev_" if where == "cuda" else "kofft_hip_"
    arena = Arena(where, f"stft_onesided ({where}) {_ids(shape)}")
    r_sig, r_win = arena.input(flat, align_off=4, row_bytes=stride * 4), arena.input(win)
    r_out = arena.output(rows * frames * k * 8, align_off=8, row_bytes=k * 8)
    fn = getattr(lib, pre + "stft_onesided_f32")
    for _ in range(2):
        assert fn(ctx, _vp(r_sig), rows, length, stride, _vp(r_win), win_len, hop, _vp(r_out), frames) == 0
        fft32.synchronize()
    arena.verify()
    got = arena.read(r_out, np.complex64, (rows, frames, k))
    assert bits_equal(got, np.stack([oracle.stft(r, win, hop, frames)[:, :k] for r in x]))


@pytest.mark.parametrize("where", ["cuda", "host"])
@pytest.mark.parametrize("win_len,hop,rows,nfr", [(1, 1, 3, 4), (16, 4, 5, 7), (15, 4, 3, 6), (256, 64, 3, 9), (1024, 256, 4, 5), (400, 160, 3, 6),
                                                  (16, 20, 3, 4)])
def test_istft_onesided_footprint(fft32, oracle, where, win_len, hop, rows, nfr):
    rng = seeded(69000 + win_len + hop)
    out_len = (nfr - 1) * hop + win_len + 3
    k = bins(win_len)
    win = rng.uniform(0.1, 1, win_len).astype(np.float32)
    half = (rng.uniform(-1, 1, (rows, nfr, k)) + 1j * rng.uniform(-1, 1, (rows, nfr, k))).astype(np.complex64)
    full = complete(half, win_len)
    zeros = np.zeros((rows, out_len), np.float32)
    want = np.stack([oracle.istft(full[r].copy(), win, hop, out_len) for r in range(rows)])
    lib, ctx, pre = fft32._lib, fft32._ctx, "kofft_hip_dev_" if where == "cuda" else "kofft_hip_"
    arena = Arena(where, f"istft_onesided ({where})")
    r_half, r_win = arena.input(half, align_off=8, row_bytes=k * 8), arena.input(win, align_off=4)
    r_out = arena.output(zeros.nbytes, prefill=zeros, row_bytes=out_len * 4)
    for _ in range(2):
        arena.restore(r_out)
        assert getattr(lib, pre + "istft_onesided_f32")(ctx, _vp(r_half), rows, nfr, _vp(r_win), win_len, hop, _vp(r_out), out_len) == 0
        fft32.synchronize()
    arena.verify()
    got = arena.read(r_out, np.float32, (rows, out_len))
    # (where every window-square sum exceeds 1e-8 -- the windows here are >= 0.1 -- inverse_parallel's sums are istft's)
    covered = np.zeros(out_len, bool)
    for f in range(nfr):
        covered[f * hop:f * hop + win_len] = True
    assert bits_equal(got[:, covered], want[:, covered]) and not got[:, ~covered].any()
