"""Guard bands (tests/redzone.py) around the buffers of the six spectrogram entry points -- magnitude_to_db, db_scale and the render, each
in its host-pointer and its device-pointer form: a call writes its output and nothing else, leaves the magnitudes, max_mag and the
bin -> pixel table as they were, and the result inside the bands is the oracle's.

Cases: picture rows whose pitch frames * 3 is not a multiple of 4 (every phase of a row against the dwords the kernel stores), outputs
at every byte offset mod 4, ragged last tiles in both directions, a last group of fewer than four pixels in the frame-major layout,
both settings of the transpose switch."""
import ctypes as C

import numpy as np
import pytest

import spectrogram_oracle as so
from conftest import seeded
from redzone import Arena
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32

# (frames, bins, depth, scale, layout, input offset, output offset in bytes)
CASES = [(65, 70, 8, 0, 1, 0, 0), (63, 64, 8, 1, 1, 4, 1), (5, 130, 8, 0, 1, 0, 2), (67, 3, 8, 1, 1, 8, 3), (130, 65, 16, 0, 1, 0, 2),
         (3, 7, 16, 1, 1, 4, 6), (65, 70, 8, 1, 0, 0, 0), (7, 9, 8, 0, 0, 4, 1), (5, 5, 16, 0, 0, 12, 2), (1, 1, 8, 0, 1, 0, 3)]


@pytest.fixture(scope="module")
def direct32():
    import kofft_amd
    from kofft_amd import spectrogram as sp

    f = kofft_amd.HipFftImpl(F)
    sp.set_transpose(False, fft=f)
    yield f
    f.close()


def _x(frames, bins, seed):
    x = (F(1.5) * (10.0 ** seeded(seed).uniform(-8.0, 0.0, (frames, bins)))).astype(F)
    x.reshape(-1)[0] = F(1.5)
    return x, F(1.5)


@pytest.mark.parametrize("frames,bins,depth,scale,layout,off_in,off_out", CASES)
@pytest.mark.parametrize("where", ["cuda", "host"])
def test_render_guard_bands(fft32, direct32, where, frames, bins, depth, scale, layout, off_in, off_out):
    x, mx = _x(frames, bins, 58000 + frames + bins)
    px = 6 if depth == 16 else 3
    name = ("kofft_hip_dev_" if where == "cuda" else "kofft_hip_") + "spectrogram_render_f32"
    want = so.render(x, mx, 0, -120.0, so.FIRE, depth, scale, layout)
    side = Arena("host", "the bin -> pixel table")  # a host pointer in both forms
    r_t = side.input(so.log_bin_map(bins), row_bytes=4 * bins)
    table = C.c_void_p(r_t.addr) if scale == 1 else None
    for f, route in ((fft32, "LDS exchange"), (direct32, "direct stores")):
        arena = Arena(where, f"{name} frames={frames} bins={bins} depth={depth} scale={scale} layout={layout} {route}")
        r_in = arena.input(x, align_off=off_in, row_bytes=4 * bins)
        r_max = arena.input(np.array([mx], F), align_off=4)
        row = (bins if layout == 0 else frames) * px
        r_out = arena.output(frames * bins * px, align_off=off_out, row_bytes=row)
        for _ in range(2):
            assert getattr(f._lib, name)(f._ctx, C.c_void_p(r_in.addr), frames, bins, C.c_void_p(r_max.addr), 0, -120.0, so.FIRE, depth, scale,
                                         layout, table, C.c_void_p(r_out.addr)) == 0
            f.synchronize()
        arena.verify()
        side.verify()
        got = arena.read(r_out, np.uint8, (frames * bins * px,))
        got = got.view(np.uint16) if depth == 16 and off_out % 2 == 0 else got
        ref = want if got.dtype == want.dtype else want.view(np.uint8)
        assert_rows_equal(got.reshape(ref.shape), ref, arena.what)


@pytest.mark.parametrize("count,off_in,off_out", [(1, 0, 0), (63, 4, 8), (65, 12, 4), (100_003, 0, 12)])
@pytest.mark.parametrize("where", ["cuda", "host"])
def test_pointwise_guard_bands(fft32, where, count, off_in, off_out):
    x = (F(1.5) * (10.0 ** seeded(59000 + count).uniform(-9.0, 0.0, count))).astype(F)
    mx = F(1.5)
    prefix = "kofft_hip_dev_" if where == "cuda" else "kofft_hip_"
    arena = Arena(where, f"{prefix}magnitude_to_db / db_scale count={count}")
    r_in = arena.input(x, align_off=off_in)
    r_max = arena.input(np.array([mx], F), align_off=8)
    r_db = arena.output(4 * count, align_off=off_out)
    r_t = arena.output(4 * count, align_off=off_out)
    for _ in range(2):
        assert getattr(fft32._lib, prefix + "magnitude_to_db_f32")(fft32._ctx, C.c_void_p(r_in.addr), count, C.c_void_p(r_max.addr), -120.0,
                                                                  C.c_void_p(r_db.addr)) == 0
        assert getattr(fft32._lib, prefix + "db_scale_f32")(fft32._ctx, C.c_void_p(r_in.addr), count, C.c_void_p(r_max.addr), 60.0,
                                                           C.c_void_p(r_t.addr)) == 0
        fft32.synchronize()
    arena.verify()
    assert_rows_equal(arena.read(r_db, F, (count,)), so.magnitude_to_db(x, mx, -120.0), arena.what + ": magnitude_to_db", nan_safe=True)
    assert_rows_equal(arena.read(r_t, F, (count,)), so.db_scale(x, mx, 60.0), arena.what + ": db_scale", nan_safe=True)
