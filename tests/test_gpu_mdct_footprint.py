"""Guard bands (tests/redzone.py) around every buffer of the fast DCT-IV, MDCT and IMDCT entries, device-pointer and
host-pointer forms: a call writes its output and nothing else, leaves its inputs and the window as they were, and the result inside the
bands is the oracle's.

Cases: ragged last workgroups of the fused kernel, rows a stride apart (the gaps are band pattern: a NaN, so a read of a neighbour's
gap shows in the result), leads 0 and 2N - 1, frames past the row's end, windows of the IMDCT that start and end inside a block,
buffers that are only 4-byte aligned, lengths only the composed route takes, both routes of the rest."""
import ctypes as C

import numpy as np
import pytest

from conftest import seeded
import mdct_oracle as mo
from redzone import Arena
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def composed32():
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_mdct_fused(False)
    yield f
    f.close()


def _routes(fft32, composed32):
    return ((fft32, "default"), (composed32, "composed"))


@pytest.mark.parametrize("n,rows,off_in,off_out", [(64, 17, 0, 0), (512, 5, 4, 12), (8192, 3, 4, 4), (6, 9, 4, 0), (960, 3, 0, 4), (16384, 2, 0, 0)])
@pytest.mark.parametrize("where", ["cuda", "host"])
def test_dct4_guard_bands(fft32, composed32, where, n, rows, off_in, off_out):
    u = seeded(13500 + n).uniform(-1, 1, (rows, n)).astype(F)
    want = mo.dct4_ref(u)
    name = "kofft_hip_dev_dct4_fast_f32" if where == "cuda" else "kofft_hip_dct4_fast_f32"
    for f, route in _routes(fft32, composed32):
        arena = Arena(where, f"{name} N={n} rows={rows} {route}")
        r_in = arena.input(u, align_off=off_in, row_bytes=4 * n)
        r_out = arena.output(4 * n * rows, align_off=off_out, row_bytes=4 * n)
        for _ in range(2):
            assert getattr(f._lib, name)(f._ctx, C.c_void_p(r_in.addr), C.c_void_p(r_out.addr), n, rows) == 0, arena.what
        arena.verify()
        assert_rows_equal(arena.read(r_out, F, (rows, n)), want, arena.what)
        if where == "cuda":  # in place: one buffer, transformed once
            arena = Arena(where, f"{name} N={n} rows={rows} {route} in place")
            r_io = arena.inout(u, align_off=off_out, row_bytes=4 * n)
            assert getattr(f._lib, name)(f._ctx, C.c_void_p(r_io.addr), C.c_void_p(r_io.addr), n, rows) == 0, arena.what
            arena.verify()
            assert_rows_equal(arena.read(r_io, F, (rows, n)), want, arena.what)


# (N, rows, nx, row stride, lead, frames, offsets of x / out in bytes)
MDCT_CASES = [(64, 7, 300, 300, 64, 6, 0, 0), (64, 5, 333, 340, 0, 8, 4, 12), (1024, 3, 3000, 3001, 2047, 5, 4, 4), (8192, 2, 20000, 20010, 8192, 4, 0, 4),
              (2, 5, 9, 11, 1, 7, 4, 0), (240, 3, 1000, 1003, 240, 6, 0, 0), (16384, 2, 40000, 40000, 16384, 4, 0, 0)]


@pytest.mark.parametrize("n,rows,nx,stride,lead,frames,off_in,off_out", MDCT_CASES)
@pytest.mark.parametrize("where", ["cuda", "host"])
def test_mdct_guard_bands(fft32, composed32, where, n, rows, nx, stride, lead, frames, off_in, off_out):
    rng = seeded(13600 + n + nx)
    x = rng.uniform(-1, 1, (rows, nx)).astype(F)
    w = rng.uniform(0.1, 1, 2 * n).astype(F)
    want = mo.mdct_ref(x, w, lead, frames).reshape(rows, frames * n)
    name = "kofft_hip_dev_mdct_f32" if where == "cuda" else "kofft_hip_mdct_f32"
    for f, route in _routes(fft32, composed32):
        arena = Arena(where, f"{name} N={n} rows={rows} nx={nx} stride={stride} lead={lead} frames={frames} {route}")
        # the gaps between the rows hold NaN and are part of the input region: never written, and not read either (the result)
        padded = np.full((rows, stride), np.nan, F)
        padded[:, :nx] = x
        r_x = arena.input(padded.reshape(-1)[:(rows - 1) * stride + nx], align_off=off_in, row_bytes=4 * stride)
        r_w = arena.input(w, align_off=off_in)
        r_out = arena.output(4 * frames * n * rows, align_off=off_out, row_bytes=4 * frames * n)
        for _ in range(2):
            rc = getattr(f._lib, name)(f._ctx, C.c_void_p(r_x.addr), rows, nx, stride, C.c_void_p(r_w.addr), n, lead, C.c_void_p(r_out.addr), frames)
            assert rc == 0, arena.what
        arena.verify()
        assert_rows_equal(arena.read(r_out, F, (rows, frames * n)), want, arena.what)


# (N, rows, frames, out_first, out_len (None: to the end), offsets of coef / out in bytes)
IMDCT_CASES = [(64, 7, 5, 0, None, 0, 0), (64, 5, 9, 64, 300, 4, 12), (1024, 3, 5, 1500, 2049, 4, 4), (8192, 2, 3, 100, 50, 0, 4),
               (2, 5, 7, 3, 9, 4, 0), (240, 3, 6, 240, 1000, 0, 0), (16384, 2, 3, 16384, 32768, 0, 0)]


@pytest.mark.parametrize("n,rows,frames,first,count,off_in,off_out", IMDCT_CASES)
@pytest.mark.parametrize("where", ["cuda", "host"])
def test_imdct_guard_bands(fft32, composed32, where, n, rows, frames, first, count, off_in, off_out):
    rng = seeded(13700 + n + frames)
    X = rng.uniform(-1, 1, (rows, frames, n)).astype(F)
    w = rng.uniform(0.1, 1, 2 * n).astype(F)
    count = (frames + 1) * n - first if count is None else count
    scale = F(2.0 / n)
    want = np.ascontiguousarray(mo.imdct_ref(X, w, scale)[:, first:first + count])
    name = "kofft_hip_dev_imdct_f32" if where == "cuda" else "kofft_hip_imdct_f32"
    for f, route in _routes(fft32, composed32):
        arena = Arena(where, f"{name} N={n} rows={rows} frames={frames} window=({first}, {count}) {route}")
        r_X = arena.input(X, align_off=off_in, row_bytes=4 * frames * n)
        r_w = arena.input(w, align_off=off_in)
        r_out = arena.output(4 * count * rows, align_off=off_out, row_bytes=4 * count)
        for _ in range(2):
            rc = getattr(f._lib, name)(f._ctx, C.c_void_p(r_X.addr), rows, frames, C.c_void_p(r_w.addr), n, C.c_float(float(scale)), C.c_void_p(r_out.addr),
                                       first, count)
            assert rc == 0, arena.what
        arena.verify()
        assert_rows_equal(arena.read(r_out, F, (rows, count)), want, arena.what)
