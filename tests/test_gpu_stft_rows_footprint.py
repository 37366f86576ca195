"""The row-wise STFT, stft_magnitudes and ISTFT entry points inside guard bands (tests/redzone.py), as test_gpu_footprint.py does for
the rest of the header: every device-pointer form with its pointers in one arena on the device, every host-pointer form in a numpy
arena through raw ctypes calls.  A call writes its outputs and nothing else and leaves its `const` inputs alone -- the inter-row gaps of
row_stride > len (NaN here) are among them -- and its results are the oracle's, bit for bit, so an over-read that reaches a result shows."""
import ctypes as C

import numpy as np
import pytest

from conftest import bits_equal, seeded
from redzone import Arena

pytestmark = pytest.mark.gpu

# (win_len, hop, rows, frames, gap): a small kernel, the generic kernel with a tile-aligned and a ragged frame count, persistent group
# kernels (rows x frames past the threshold), one wavefront and several per transform, the composed route
SHAPES = [(16, 4, 5, 7, 5), (64, 16, 3, 16, 0), (256, 64, 7, 5, 3), (256, 64, 2731, 12, 5), (1024, 256, 3, 5, 5), (1024, 256, 1639, 5, 0),
          (4096, 1024, 3, 3, 1), (400, 160, 5, 6, 5)]


def _ids(s):
    return "win%d-hop%d-rows%d-frames%d-gap%d" % s


def _signal(rng, rows, length, stride):
    x = rng.uniform(-1, 1, (rows, length)).astype(np.float32)
    host = np.full((rows, stride), np.nan, np.float32)
    host[:, :length] = x
    return x, host.reshape(-1)[:(rows - 1) * stride + length]


def _vp(r):
    return C.c_void_p(int(r))


@pytest.mark.parametrize("where", ["cuda", "host"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_stft_and_magnitudes_rows_footprint(fft32, oracle, where, shape):
    import kofft_amd

    win_len, hop, rows, frames, gap = shape
    length, stride = frames * hop - 1, frames * hop - 1 + gap
    rng = seeded(61000 + win_len + rows)
    x, flat = _signal(rng, rows, length, stride)
    win = rng.uniform(0.1, 1, win_len).astype(np.float32)
    lib, ctx, pre = fft32._lib, fft32._ctx, "kofft_hip_dev_" if where == "cuda" else "kofft_hip_"
    # STFT
    arena = Arena(where, f"stft_rows ({where}) {_ids(shape)}")
    r_sig, r_win = arena.input(flat, align_off=4, row_bytes=stride * 4), arena.input(win)
    r_out = arena.output(rows * frames * win_len * 8, row_bytes=win_len * 8)
    fn = getattr(lib, pre + "stft_rows_f32")
    for _ in range(2):
        assert fn(ctx, _vp(r_sig), rows, length, stride, _vp(r_win), win_len, hop, _vp(r_out), frames) == 0
        fft32.synchronize()
    arena.verify()
    got = arena.read(r_out, np.complex64, (rows, frames, win_len))
    assert bits_equal(got, np.stack([oracle.stft(r, win, hop, frames) for r in x]))
    # magnitudes
    arena = Arena(where, f"stft_magnitudes_rows ({where}) {_ids(shape)}")
    r_sig = arena.input(flat, align_off=8, row_bytes=stride * 4)
    r_mag = arena.output(rows * frames * (win_len // 2) * 4, row_bytes=(win_len // 2) * 4)
    r_max = arena.output(rows * 4, align_off=4)
    fn = getattr(lib, pre + "stft_magnitudes_rows_f32")
    for _ in range(2):
        assert fn(ctx, _vp(r_sig), rows, length, stride, win_len, hop, _vp(r_mag), frames, _vp(r_max)) == 0
        fft32.synchronize()
    arena.verify()
    want = [oracle.stft_magnitudes(r, win_len, hop) for r in x]
    assert bits_equal(arena.read(r_mag, np.float32, (rows, frames, win_len // 2)), np.stack([m for m, _ in want]))
    assert bits_equal(arena.read(r_max, np.float32, (rows,)), np.array([v for _, v in want], np.float32))


@pytest.mark.parametrize("where", ["cuda", "host"])
@pytest.mark.parametrize("win_len,hop,rows,nfr", [(16, 4, 5, 7), (256, 64, 3, 9), (1024, 256, 4, 5), (400, 160, 3, 6), (16, 20, 3, 4)])
def test_istft_rows_footprint(fft32, oracle, where, win_len, hop, rows, nfr):
    rng = seeded(62000 + win_len + hop)
    out_len = (nfr - 1) * hop + win_len + 3
    win = rng.uniform(0.1, 1, win_len).astype(np.float32)
    spec = (rng.uniform(-1, 1, (rows, nfr, win_len)) + 1j * rng.uniform(-1, 1, (rows, nfr, win_len))).astype(np.complex64)
    zeros = np.zeros((rows, out_len), np.float32)
    want = np.stack([oracle.istft(spec[r], win, hop, out_len) for r in range(rows)])
    lib, ctx, pre = fft32._lib, fft32._ctx, "kofft_hip_dev_" if where == "cuda" else "kofft_hip_"
    # mode 1: the frames are transformed in place, output accumulated into (from zero here), scratch written
    arena = Arena(where, f"istft_rows ({where})")
    r_fr, r_win = arena.inout(spec, row_bytes=win_len * 8), arena.input(win, align_off=4)
    r_out, r_scr = arena.output(zeros.nbytes, prefill=zeros, row_bytes=out_len * 4), arena.output(zeros.nbytes, align_off=8, row_bytes=out_len * 4)
    assert getattr(lib, pre + "istft_rows_f32")(ctx, _vp(r_fr), rows, nfr, _vp(r_win), win_len, hop, _vp(r_out), out_len,
                                                             _vp(r_scr), out_len) == 0
    fft32.synchronize()
    arena.verify()
    assert bits_equal(arena.read(r_out, np.float32, (rows, out_len)), want)
    # mode 2: the frames are an input
    arena = Arena(where, f"istft_parallel_rows ({where})")
    r_fr, r_win = arena.input(spec, row_bytes=win_len * 8), arena.input(win, align_off=4)
    r_out = arena.output(zeros.nbytes, prefill=zeros, row_bytes=out_len * 4)
    for _ in range(2):
        arena.restore(r_out)
        assert getattr(lib, pre + "istft_parallel_rows_f32")(ctx, _vp(r_fr), rows, nfr, _vp(r_win), win_len, hop, _vp(r_out),
                                                                          out_len) == 0
        fft32.synchronize()
    arena.verify()
    got = arena.read(r_out, np.float32, (rows, out_len))
    # (where every window-square sum exceeds 1e-8 -- the windows here are >= 0.1 -- inverse_parallel's sums are istft's)
    covered = np.zeros(out_len, bool)
    for f in range(nfr):
        covered[f * hop:f * hop + win_len] = True
    assert bits_equal(got[:, covered], want[:, covered]) and not got[:, ~covered].any()
