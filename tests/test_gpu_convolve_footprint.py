"""Guard bands (tests/redzone.py) around the signal, the taps and the output of kofft_hip_convolve_f32 and kofft_hip_dev_convolve_f32: a
call writes rows x out_len floats and nothing else, leaves its inputs as they were, and the result inside the bands is the oracle's.

Cases: a ragged last workgroup of the fused kernel, a window that starts and ends mid-block, per-row filters, 4-byte aligned buffers,
the correlate flag, a block only the composed route takes, both routes of the rest."""
import ctypes as C

import numpy as np
import pytest

from conftest import seeded
from convolve_oracle import convolve_ref
from redzone import Arena
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32

# (block, rows, nx, nh, per-row filters, correlate, first, count (None: to the end), offsets of x / out in bytes)
CASES = [(32, 7, 100, 9, False, False, 0, None, 0, 0),
         (64, 5, 333, 17, True, False, 50, 201, 4, 12),      # a window from mid-block to mid-block, per-row filters
         (256, 3, 700, 65, False, True, 391, 1, 0, 4),       # one sample
         (1024, 5, 4000, 257, True, True, 128, 4000, 8, 0),  # "same"
         (4096, 3, 9000, 1025, False, False, 1024, 7976, 4, 4),  # "valid"
         (8, 9, 50, 3, True, False, 5, 40, 4, 4),            # composed only
         (8192, 2, 13000, 100, False, False, 8000, 5099, 0, 0)]  # composed only, the last blocks


@pytest.fixture(scope="module")
def composed32():
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_convolve_fused(False)
    yield f
    f.close()


@pytest.mark.parametrize("block,rows,nx,nh,per_row,correlate,first,count,off_in,off_out", CASES)
@pytest.mark.parametrize("where", ["cuda", "host"])
def test_guard_bands(fft32, composed32, where, block, rows, nx, nh, per_row, correlate, first, count, off_in, off_out):
    rng = seeded(10500 + block + nx)
    x = rng.uniform(-1, 1, (rows, nx)).astype(F)
    h = rng.uniform(-1, 1, (rows, nh) if per_row else nh).astype(F)
    full = nx + nh - 1
    count = full - first if count is None else count
    want = np.ascontiguousarray(convolve_ref(x, h, block, correlate)[:, first:first + count])
    name = "kofft_hip_dev_convolve_f32" if where == "cuda" else "kofft_hip_convolve_f32"
    for f, route in ((fft32, "default"), (composed32, "composed")):
        arena = Arena(where, f"{name} block={block} rows={rows} nx={nx} nh={nh} per_row={per_row} window=({first}, {count}) {route}")
        r_x = arena.input(x, align_off=off_in, row_bytes=4 * nx)
        r_h = arena.input(h, align_off=off_in, row_bytes=4 * nh)
        r_out = arena.output(4 * count * rows, align_off=off_out, row_bytes=4 * count)
        for _ in range(2):
            rc = getattr(f._lib, name)(f._ctx, C.c_void_p(r_x.addr), rows, nx, C.c_void_p(r_h.addr), rows if per_row else 1, nh, block,
                                       1 if correlate else 0, C.c_void_p(r_out.addr), first, count)
            assert rc == 0, arena.what
        arena.verify()
        assert_rows_equal(arena.read(r_out, F, (rows, count)), want, arena.what)
