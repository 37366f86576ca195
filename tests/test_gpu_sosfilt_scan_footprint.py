"""Guard bands (tests/redzone.py) around the signal, the coefficients, both states and the output of kofft_hip_sosfilt_scan_f32 and
kofft_hip_dev_sosfilt_scan_f32: a call writes rows x nx floats and rows x sections x 2 floats of state and nothing else, leaves its
inputs as they were, and the result inside the bands is the oracle's.

Every case has three rows of a length that is no multiple of the chunk or the tile: the last chunk of a row is short, its last tile
too, and a wavefront holds the chunks of all three rows, so a wrong mask or a wrong virtual-row address reads or writes a neighbouring
row or a band.  Both entry points, forward and reverse, buffers offset by 0, 4 and 12 bytes, one and two groups of sections, rows of
one chunk and of several."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import seeded
from redzone import Arena
from rowcheck import assert_rows_equal
from sosfilt_oracle import cascade
from sosfilt_scan_oracle import sosfilt_scan_ref

pytestmark = pytest.mark.gpu
F = np.float32


def _define(name):
    from kofft_amd import _lib

    return int(re.search(rf"#define KOFFT_HIP_SOSFILT_{name} (\d+)", _lib.HEADER_PATH.read_text()).group(1))


T = _define("TILE")
G = _define("GROUP")

# (nx, chunk, sections, offset of every buffer in bytes)
CASES = [(5 * T + 5, T, 2, 0), (30 * T - 3, 2 * T, 3, 4), (7 * T + 1, 3 * T, G + 1, 12), (T - 3, T, 1, 4), (1, 2 * T, 1, 12)]


@pytest.mark.parametrize("nx,chunk,sections,off", CASES)
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("where", ["cuda", "host"])
def test_guard_bands(fft32, where, reverse, nx, chunk, sections, off):
    rows = 3
    rng = seeded(32200 + nx + sections)
    x = rng.uniform(-1, 1, (rows, nx)).astype(F)
    zi = rng.uniform(-1, 1, (rows, sections, 2)).astype(F)
    sos = cascade(sections)
    want_y, want_z = sosfilt_scan_ref(sos, x, chunk, zi, reverse)
    name = "kofft_hip_dev_sosfilt_scan_f32" if where == "cuda" else "kofft_hip_sosfilt_scan_f32"
    f = fft32
    arena = Arena(where, f"{name} rows={rows} nx={nx} chunk={chunk} sections={sections} reverse={reverse} off={off}")
    r_x = arena.input(x, align_off=off, row_bytes=4 * nx, name="x")
    r_sos = arena.input(sos, align_off=off, row_bytes=24, name="sos")
    r_zi = arena.input(zi, align_off=off, row_bytes=8 * sections, name="zi")
    r_zf = arena.output(8 * sections * rows, align_off=off, row_bytes=8 * sections, name="zf")
    r_out = arena.output(4 * nx * rows, align_off=off, row_bytes=4 * nx, name="out")
    for _ in range(2):
        rc = getattr(f._lib, name)(f._ctx, C.c_void_p(r_x.addr), rows, nx, C.c_void_p(r_sos.addr), sections, C.c_void_p(r_zi.addr),
                                   C.c_void_p(r_zf.addr), chunk, 1 if reverse else 0, C.c_void_p(r_out.addr))
        assert rc == 0, arena.what
        if where == "cuda":
            f.synchronize()
    arena.verify()
    assert_rows_equal(arena.read(r_out, F, (rows, nx)), want_y, arena.what)
    assert_rows_equal(arena.read(r_zf, F, (rows, 2 * sections)), want_z.reshape(rows, -1), arena.what + ": final states")
