"""Guard bands (tests/redzone.py) around the signals, the window and the output of kofft_hip_welch_f32, kofft_hip_csd_f32 and their
kofft_hip_dev_* forms: a call writes rows x K floats (complex values) and nothing else, leaves its inputs as they were, and the result
inside the bands is the oracle's.

Cases: one group per row (the fused kernel stores the scaled totals itself), several groups with a short last one (the running total
lives in the output between the kernels), a ragged last workgroup, 4-byte aligned buffers, a null window, a window length only the
composed route takes, both routes of the rest."""
import ctypes as C

import numpy as np
import pytest

import welch_oracle as wo
from redzone import Arena
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32

# (win_len, hop, rows, frames, a caller's window, flags, offsets of the signals / the output in bytes)
CASES = [(64, 16, 7, 20, True, 0, 0, 0),
         (64, 1, 5, 65, False, 1, 4, 12),
         (256, 64, 3, 33, True, 1, 0, 4),
         (1024, 256, 5, 70, False, 0, 8, 0),
         (4096, 1024, 3, 40, True, 1, 4, 4),
         (400, 160, 4, 45, True, 1, 4, 4),     # composed only (Bluestein)
         (6, 2, 9, 70, False, 0, 0, 4)]        # composed only


@pytest.fixture(scope="module")
def composed32():
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_welch_fused(0)
    yield f
    f.close()


@pytest.fixture(scope="module")
def fused32():
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_welch_fused(2)
    yield f
    f.close()


@pytest.mark.parametrize("win_len,hop,rows,frames,own_window,flags,off_in,off_out", CASES)
@pytest.mark.parametrize("csd", [False, True])
@pytest.mark.parametrize("where", ["cuda", "host"])
def test_guard_bands(fused32, composed32, oracle, where, csd, win_len, hop, rows, frames, own_window, flags, off_in, off_out):
    x = wo.grid_input(win_len, hop, frames, rows)
    y = wo.grid_input(win_len, hop, frames, rows, 1) if csd else None
    win = oracle.hann(win_len)
    if own_window:
        win = np.ascontiguousarray(win * F(0.5) + F(0.25), F)
    length, K = x.shape[1], win_len // 2 + 1
    want = wo.welch_ref(x, win, hop, frames, 0.3, bool(flags), y=y)
    stem = "csd_f32" if csd else "welch_f32"
    name = f"kofft_hip_dev_{stem}" if where == "cuda" else f"kofft_hip_{stem}"
    for f, route in ((fused32, "fused"), (composed32, "composed")):
        arena = Arena(where, f"{name} win_len={win_len} hop={hop} rows={rows} frames={frames} {route}")
        r_x = arena.input(x, align_off=off_in, row_bytes=4 * length)
        r_y = arena.input(y, align_off=off_in, row_bytes=4 * length) if csd else None
        r_w = arena.input(win, align_off=off_in, row_bytes=4 * win_len) if own_window else None
        out_row = K * (8 if csd else 4)
        r_out = arena.output(out_row * rows, align_off=off_out, row_bytes=out_row)
        sigs = [C.c_void_p(r_x.addr)] + ([C.c_void_p(r_y.addr)] if csd else [])
        for _ in range(2):
            rc = getattr(f._lib, name)(f._ctx, *sigs, rows, length, length, C.c_void_p(r_w.addr) if own_window else None, win_len, hop,
                                       frames, 0.3, flags, C.c_void_p(r_out.addr))
            assert rc == 0, arena.what
            f.synchronize()
        arena.verify()
        assert_rows_equal(arena.read(r_out, np.complex64 if csd else F, (rows, K)), want, arena.what)
