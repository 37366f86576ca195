"""Guard bands (tests/redzone.py) around the signal, the window and the outputs of the four audio front-end entry points
(kofft_hip_stft_mel_f32, kofft_hip_stft_mfcc_f32, kofft_hip_dev_stft_mel_f32, kofft_hip_dev_stft_mfcc_f32), on the fused kernel
wherever it fits and on the composed route: a call writes its output and nothing else, leaves its inputs as they were,
and the result inside the bands is the oracle's.

Cases: ragged last workgroups (rows * frames not a multiple of the frames per workgroup), frames that run off the end of the last row
right in front of a band, 4-byte aligned signals and outputs, a caller's window and the default one, a Bluestein length."""
import ctypes as C

import numpy as np
import pytest

import frontend_oracle as fo
from conftest import seeded
from redzone import Arena
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32

# (win_len, hop, rows, frames, num_mel, num_coeffs, a caller's window, signal offset, output offset in bytes)
CASES = [(64, 16, 3, 17, 8, 5, False, 0, 0), (128, 128, 2, 15, 26, 13, True, 4, 0), (256, 64, 1, 33, 40, 13, False, 0, 12),
         (512, 200, 3, 5, 26, 26, True, 8, 4), (1024, 256, 2, 9, 40, 13, False, 4, 4), (2048, 512, 3, 3, 128, 13, True, 0, 0),
         (400, 160, 2, 7, 13, 13, True, 4, 8), (32, 8, 2, 9, 4, 2, False, 0, 0)]


@pytest.fixture(scope="module")
def composed32():
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_frontend_fused(0)
    yield f
    f.close()


@pytest.fixture(scope="module")
def forced32():
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_frontend_fused(2)
    yield f
    f.close()


def _call(f, name, sig, rows, length, win, win_len, hop, frames, bins, out, nc):
    b = np.ascontiguousarray(bins, np.uint64)
    args = [f._ctx, C.c_void_p(sig), rows, length, length, C.c_void_p(win) if win else None, win_len, hop, frames, C.c_void_p(b.ctypes.data),
            b.size - 2]
    if "mfcc" in name:
        args.append(nc)
    return getattr(f._lib, name)(*args, C.c_void_p(out))


@pytest.mark.parametrize("win_len,hop,rows,frames,num_mel,nc,windowed,off_in,off_out", CASES)
@pytest.mark.parametrize("where", ["cuda", "host"])
def test_guard_bands(composed32, forced32, oracle, where, win_len, hop, rows, frames, num_mel, nc, windowed, off_in, off_out):
    from kofft_amd import mfcc, window

    length = frames * hop - hop // 3
    bins = [int(b) for b in mfcc.mel_bins(16000.0, win_len // 2, num_mel)]
    x = fo.signal(seeded(51000 + win_len), rows, length, special=False)
    win = window.hamming(win_len) if windowed else None
    want_e, want_c = fo.expected(oracle, x, win_len, hop, frames, bins, win)
    prefix = "kofft_hip_dev_" if where == "cuda" else "kofft_hip_"
    for f, route in ((forced32, "fused where it fits"), (composed32, "composed")):
        arena = Arena(where, f"{prefix}stft_mel/mfcc win_len={win_len} hop={hop} rows={rows} frames={frames} num_mel={num_mel} nc={nc} {route}")
        r_in = arena.input(x, align_off=off_in, row_bytes=4 * length)
        r_w = arena.input(win, align_off=off_in, row_bytes=4 * win_len) if windowed else None
        r_e = arena.output(4 * num_mel * rows * frames, align_off=off_out, row_bytes=4 * num_mel)
        r_c = arena.output(4 * nc * rows * frames, align_off=off_out, row_bytes=4 * nc)
        w_addr = r_w.addr if windowed else 0
        for _ in range(2):
            assert _call(f, prefix + "stft_mel_f32", r_in.addr, rows, length, w_addr, win_len, hop, frames, bins, r_e.addr, 0) == 0
            assert _call(f, prefix + "stft_mfcc_f32", r_in.addr, rows, length, w_addr, win_len, hop, frames, bins, r_c.addr, nc) == 0
        arena.verify()
        assert_rows_equal(arena.read(r_e, F, (rows * frames, num_mel)), want_e.reshape(-1, num_mel), arena.what + ": energies", nan_safe=True)
        assert_rows_equal(arena.read(r_c, F, (rows * frames, nc)), np.ascontiguousarray(want_c[:, :, :nc]).reshape(-1, nc),
                          arena.what + ": coefficients", nan_safe=True)
