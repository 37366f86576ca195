"""Guard bands (tests/redzone.py) around the signal, the bank and the output of kofft_hip_convolve_bank_f32 and
kofft_hip_dev_convolve_bank_f32: a call writes rows x filters x out_len elements and nothing else, leaves its inputs as they were, and
the result inside the bands is the oracle's.

Cases: a ragged last workgroup of the fused kernel, a window that starts and ends mid-block, one sample, "same" and "valid", real and
complex taps, the three output kinds (8-byte elements for the complex one), 4-byte aligned buffers, the correlate flag, blocks only the
composed route takes, both routes of the rest."""
import ctypes as C

import numpy as np
import pytest

from conftest import seeded
from convolve_bank_oracle import KINDS, convolve_bank_ref
from redzone import Arena
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32

# (block, rows, nx, filters, nh, complex taps, correlate, first, count (None: to the end), offsets of x / out in bytes)
CASES = [(32, 7, 100, 3, 9, False, False, 0, None, 0, 0),
         (64, 5, 333, 2, 17, True, False, 50, 201, 4, 8),       # a window from mid-block to mid-block
         (256, 3, 700, 3, 65, False, True, 391, 1, 0, 8),        # one sample
         (1024, 3, 4000, 2, 257, True, True, 128, 4000, 8, 0),   # "same"
         (4096, 3, 9000, 2, 1025, True, False, 1024, 7976, 4, 16),  # "valid"
         (8, 9, 50, 5, 3, True, False, 5, 40, 4, 8),             # composed only
         (8192, 2, 13000, 2, 100, False, False, 8000, 5099, 0, 0)]  # composed only, the last blocks


@pytest.fixture(scope="module")
def composed32():
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_convolve_bank_fused(False)
    yield f
    f.close()


@pytest.mark.parametrize("block,rows,nx,filters,nh,cplx,correlate,first,count,off_in,off_out", CASES)
@pytest.mark.parametrize("where", ["cuda", "host"])
def test_guard_bands(fft32, composed32, where, block, rows, nx, filters, nh, cplx, correlate, first, count, off_in, off_out):
    rng = seeded(12500 + block + nx)
    x = rng.uniform(-1, 1, (rows, nx)).astype(F)
    h = rng.uniform(-1, 1, (filters, nh)).astype(F)
    if cplx:
        h = (h + 1j * rng.uniform(-1, 1, (filters, nh)).astype(F)).astype(np.complex64)
    full = nx + nh - 1
    count = full - first if count is None else count
    name = "kofft_hip_dev_convolve_bank_f32" if where == "cuda" else "kofft_hip_convolve_bank_f32"
    for kind, out in enumerate(KINDS):
        want = np.ascontiguousarray(convolve_bank_ref(x, h, block, correlate, out)[:, :, first:first + count])
        elem = want.dtype.itemsize
        flags = (1 if correlate else 0) | (2 if cplx else 0) | (kind << 2)
        for f, route in ((fft32, "default"), (composed32, "composed")):
            arena = Arena(where, f"{name} block={block} rows={rows} nx={nx} filters={filters} nh={nh} complex taps={cplx} out={out} "
                                 f"window=({first}, {count}) {route}")
            r_x = arena.input(x, align_off=off_in, row_bytes=4 * nx)
            r_h = arena.input(h, align_off=off_in, row_bytes=h.dtype.itemsize * nh)
            # (off_out is the complex kind's, a multiple of its 8-byte element; the 4-byte kinds get half of it)
            r_out = arena.output(elem * count * filters * rows, align_off=off_out * elem // 8, row_bytes=elem * count)
            for _ in range(2):
                rc = getattr(f._lib, name)(f._ctx, C.c_void_p(r_x.addr), rows, nx, C.c_void_p(r_h.addr), filters, nh, block, flags,
                                           C.c_void_p(r_out.addr), first, count)
                assert rc == 0, arena.what
            arena.verify()
            assert_rows_equal(arena.read(r_out, want.dtype, (rows, filters, count)), want, arena.what)
