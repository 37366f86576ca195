"""Guard bands (tests/redzone.py) around the signal, the window, the maxima and the pictures of kofft_hip_stft_picture_f32 and
kofft_hip_dev_stft_picture_f32: a call writes its pictures and max_out and nothing else, leaves its inputs as they were (DESIGN.md
9.2), and the result inside the bands is the oracle's.

Cases: both routes of the row maximum (one chunk: the chain's kernels; many chunks, under KOFFT_HIP_SCRATCH_CHUNK_MB=1: the max-only
pass, then windows of the pictures chunk by chunk) and the running maximum, both layouts, the pictures at byte offsets 0 .. 3, picture
pitches that are no multiple of 4 (odd frame counts at 3 bytes per pixel), max_out given and null, a caller's window and the default."""
import ctypes as C

import numpy as np
import pytest

import frontend_oracle as fo
import picture_oracle as po
import spectrogram_oracle as so
from conftest import seeded
from redzone import Arena
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32
KNOB = "KOFFT_HIP_SCRATCH_CHUNK_MB"

# (win_len, hop, rows, frames, max_mode, layout, (depth, channels), a caller's window, max_out given, signal offset, picture offset in bytes)
SMALL = [(64, 16, 3, 17, 0, 1, (8, 3), False, True, 0, 1), (128, 128, 2, 15, 1, 0, (8, 4), True, False, 4, 2), (256, 64, 1, 33, 2, 1, (16, 3), False, True, 0, 3),
         (512, 200, 3, 5, 1, 1, (8, 3), True, True, 8, 1), (1024, 256, 2, 9, 0, 0, (8, 3), False, False, 4, 3), (400, 160, 2, 7, 0, 1, (8, 3), True, True, 4, 2),
         (32, 8, 2, 67, 2, 1, (8, 4), False, True, 0, 0), (2, 1, 2, 65, 1, 1, (8, 3), False, True, 0, 1)]
# more than one chunk of 1 MiB: seams inside rows
CHUNKED = [(1024, 256, 3, 601, 0, 1, (8, 3), False, True, 0, 1), (1024, 256, 3, 601, 1, 1, (8, 3), False, True, 4, 3),
           (256, 64, 2, 1501, 0, 0, (8, 3), True, False, 0, 2), (256, 64, 3, 1001, 2, 1, (16, 3), False, True, 0, 3)]


def _run(f, oracle, where, case, route):
    from kofft_amd import window

    win_len, hop, rows, frames, max_mode, layout, (depth, channels), windowed, want_max, off_in, off_out = case
    length = frames * hop - hop // 3
    assert -(-length // hop) == frames
    bins = win_len // 2
    x = fo.signal(seeded(72000 + win_len + frames), rows, length, special=False)
    win = window.hamming(win_len) if windowed else None
    max_in = np.linspace(2.0, 9.0, rows).astype(F)
    kw = dict(max_mode=max_mode, mode=0, level=-90.0, cmap=so.RAINBOW, depth=depth, channels=channels, scale=0, layout=layout)
    want, want_mx, _ = po.expected(oracle, x, win_len, hop, frames, win, max_in=max_in, **kw)
    px = channels * depth // 8
    line = (bins if layout == 0 else frames) * px
    prefix = "kofft_hip_dev_" if where == "cuda" else "kofft_hip_"
    arena = Arena(where, f"{prefix}stft_picture_f32 {case} {route}")
    r_in = arena.input(x, align_off=off_in, row_bytes=4 * length)
    r_w = arena.input(win, align_off=off_in, row_bytes=4 * win_len) if windowed else None
    r_mi = arena.input(max_in, align_off=4, row_bytes=4) if max_mode == 2 else None
    r_mo = arena.output(4 * rows, align_off=4, row_bytes=4) if want_max else None
    r_out = arena.output(want.nbytes, align_off=off_out, row_bytes=line)
    vp = lambda r: C.c_void_p(r.addr) if r is not None else None
    for _ in range(2):
        rc = getattr(f._lib, prefix + "stft_picture_f32")(f._ctx, vp(r_in), rows, length, length, vp(r_w), win_len, hop, frames, max_mode, vp(r_mi),
                                                          vp(r_mo), 0, -90.0, so.RAINBOW, depth, channels, 0, layout, None, vp(r_out))
        assert rc == 0, arena.what
        f.synchronize()
    arena.verify()
    got = arena.read(r_out, want.dtype, want.shape)
    assert_rows_equal(got.reshape(-1, line // want.dtype.itemsize), want.reshape(-1, line // want.dtype.itemsize), arena.what)
    if want_max:
        assert arena.read(r_mo, F, (rows,)).tobytes() == want_mx.tobytes(), arena.what


@pytest.mark.parametrize("case", SMALL, ids=[f"w{c[0]}-m{c[4]}-l{c[5]}" for c in SMALL])
@pytest.mark.parametrize("where", ["cuda", "host"])
def test_guard_bands_one_chunk(fft32, oracle, where, case):
    _run(fft32, oracle, where, case, "one chunk")


@pytest.mark.parametrize("case", CHUNKED, ids=[f"w{c[0]}-m{c[4]}-l{c[5]}" for c in CHUNKED])
@pytest.mark.parametrize("where", ["cuda", "host"])
def test_guard_bands_many_chunks(monkeypatch, oracle, where, case):
    import kofft_amd

    win_len, _, rows, frames = case[:4]
    assert rows * frames * (win_len // 2) * 4 > 1 << 20 and frames % 2 == 1 and (frames * 3) % 4
    monkeypatch.setenv(KNOB, "1")
    f = kofft_amd.HipFftImpl(F)
    try:
        _run(f, oracle, where, case, "1 MiB chunks")
    finally:
        f.close()
