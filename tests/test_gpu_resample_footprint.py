"""Guard bands (tests/redzone.py) around the signal, the taps and the output of kofft_hip_resample_f32 and kofft_hip_dev_resample_f32: a
call writes rows x out_len floats and nothing else, leaves its inputs as they were, and the result inside the bands is the oracle's.

Every case has three rows and outputs whose terms run off both ends of a row: a tile's staged samples begin before the row's first
sample and end after its last, so a wrong bounds test reads row r - 1, row r + 1 or the band and changes the result.  Cases: both
routes of a tiled shape, a ragged last tile, a window, 4-byte aligned buffers, the rates of the audio conversions, a shape only the
plain kernel takes."""
import ctypes as C

import numpy as np
import pytest

from conftest import seeded
from redzone import Arena
from resample_oracle import full_len, resample_ref
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32

# (up, down, rows, nx, nh, t0, out_len (None: to the end of the full result), offsets of the inputs / the output in bytes)
CASES = [(1, 1, 3, 100, 9, 0, None, 0, 0),
         (3, 2, 3, 1500, 31, 0, None, 4, 12),        # three tiles per row, the last ragged
         (1, 3, 3, 3100, 61, 30, 1034, 0, 4),        # resample_poly's window, two tiles
         (160, 441, 3, 3000, 8821, 4410, 1089, 8, 0),  # 44.1 -> 16 kHz with the designed length
         (3, 1, 3, 400, 61, 7, 1150, 4, 4),
         (7, 5, 3, 50, 3, 0, None, 4, 4),            # up > nh
         (3, 2, 3, 700, 20001, 0, None, 0, 0)]       # the plain kernel on both contexts


@pytest.fixture(scope="module")
def plain32():
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_resample_tiled(False)
    yield f
    f.close()


@pytest.mark.parametrize("up,down,rows,nx,nh,t0,out_len,off_in,off_out", CASES)
@pytest.mark.parametrize("where", ["cuda", "host"])
def test_guard_bands(fft32, plain32, where, up, down, rows, nx, nh, t0, out_len, off_in, off_out):
    rng = seeded(28300 + up + nx)
    x = rng.uniform(-1, 1, (rows, nx)).astype(F)
    h = rng.uniform(-1, 1, nh).astype(F)
    if out_len is None:
        out_len = full_len(nx, nh, up, down)
    assert t0 + (out_len - 1) * down < (nx - 1) * up + nh
    want = resample_ref(x, h, up, down, t0, out_len)
    name = "kofft_hip_dev_resample_f32" if where == "cuda" else "kofft_hip_resample_f32"
    for f, route in ((fft32, "default"), (plain32, "plain")):
        arena = Arena(where, f"{name} up={up} down={down} rows={rows} nx={nx} nh={nh} window=({t0}, {out_len}) {route}")
        r_x = arena.input(x, align_off=off_in, row_bytes=4 * nx)
        r_h = arena.input(h, align_off=off_in, row_bytes=4 * nh)
        r_out = arena.output(4 * out_len * rows, align_off=off_out, row_bytes=4 * out_len)
        for _ in range(2):
            rc = getattr(f._lib, name)(f._ctx, C.c_void_p(r_x.addr), rows, nx, C.c_void_p(r_h.addr), nh, up, down, t0,
                                       C.c_void_p(r_out.addr), out_len)
            assert rc == 0, arena.what
        arena.verify()
        assert_rows_equal(arena.read(r_out, F, (rows, out_len)), want, arena.what)
