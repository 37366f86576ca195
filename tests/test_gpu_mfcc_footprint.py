"""Guard bands (tests/redzone.py) around the inputs and outputs of the four mel / MFCC entry points: each call writes its output and
nothing else, leaves its input as it was, and the result inside the bands is the oracle's.  Then the overlap refusal of the
device-pointer forms, which must leave both buffers untouched, followed by one valid call.

Cases: ragged last workgroups (rows not a multiple of 64), 4-byte aligned inputs and outputs, rows of an odd length, a partial output
tile (num_mel and num_coeffs not multiples of 32), both routes of the MFCC."""
import ctypes as C

import numpy as np
import pytest

import mel_oracle as mo
from conftest import seeded
from redzone import Arena
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32


def _spread(n_fft, num_mel):
    return [(i * (n_fft + 3)) // (num_mel + 1) for i in range(num_mel + 2)]  # the last edge lies beyond the row


# (n_fft, rows, num_mel, num_coeffs, input offset, output offset in bytes)
CASES = [(64, 65, 5, 3, 0, 0), (64, 130, 40, 13, 4, 0), (33, 70, 7, 7, 0, 12), (256, 129, 26, 13, 0, 4), (7, 3, 3, 1, 8, 8),
         (100, 64, 70, 33, 0, 0), (96, 67, 130, 50, 0, 0)]


@pytest.fixture(scope="module")
def composed32():
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_mfcc_fused(0)
    yield f
    f.close()


@pytest.fixture(scope="module")
def forced32():
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_mfcc_fused(2)
    yield f
    f.close()


def _x(n_fft, rows, seed):
    x = np.abs(seeded(seed).standard_normal((rows, n_fft))).astype(F)
    x[0, 0] = -0.0
    return x


def _call(f, name, p_in, p_out, n_fft, rows, bins, nc):
    b = np.ascontiguousarray(bins, np.uint64)
    args = [f._ctx, C.c_void_p(p_in), C.c_void_p(p_out), n_fft, rows, C.c_void_p(b.ctypes.data), b.size - 2]
    if "mfcc" in name:
        args.append(nc)
    return getattr(f._lib, name)(*args)


@pytest.mark.parametrize("n_fft,rows,num_mel,nc,off_in,off_out", CASES)
@pytest.mark.parametrize("where", ["cuda", "host"])
def test_guard_bands(composed32, forced32, where, n_fft, rows, num_mel, nc, off_in, off_out):
    bins = _spread(n_fft, num_mel)
    x = _x(n_fft, rows, 38000 + n_fft + num_mel)
    prefix = "kofft_hip_dev_" if where == "cuda" else "kofft_hip_"
    want_e, want_c = mo.energies(x, bins), mo.mfcc(x, bins, nc)
    for f, route in ((forced32, "fused where it fits"), (composed32, "composed")):
        arena = Arena(where, f"{prefix}mel/mfcc n_fft={n_fft} rows={rows} num_mel={num_mel} nc={nc} {route}")
        r_in = arena.input(x, align_off=off_in, row_bytes=4 * n_fft)
        r_e = arena.output(4 * num_mel * rows, align_off=off_out, row_bytes=4 * num_mel)
        r_c = arena.output(4 * nc * rows, align_off=off_out, row_bytes=4 * nc)
        for _ in range(2):
            assert _call(f, prefix + "mel_filterbank_f32", r_in.addr, r_e.addr, n_fft, rows, bins, 0) == 0
            assert _call(f, prefix + "mfcc_f32", r_in.addr, r_c.addr, n_fft, rows, bins, nc) == 0
        arena.verify()
        assert_rows_equal(arena.read(r_e, F, (rows, num_mel)), want_e, arena.what + ": energies", nan_safe=True)
        assert_rows_equal(arena.read(r_c, F, (rows, nc)), want_c, arena.what + ": coefficients", nan_safe=True)


def test_overlap_is_refused_and_nothing_is_touched(fft32):
    n_fft, rows, bins, nc = 64, 70, [0, 9, 20, 40, 64], 2
    x = _x(n_fft, rows, 39000)
    arena = Arena("cuda", "overlap refusal")
    r = arena.inout(x, row_bytes=4 * n_fft)
    r_out = arena.output(4 * 3 * rows, row_bytes=12)
    # an output inside the input, at its start, at its last float; an input inside the output
    for out in (r.addr, r.addr + 4 * 100, r.addr + 4 * (rows * n_fft - 1)):
        assert _call(fft32, "kofft_hip_dev_mel_filterbank_f32", r.addr, out, n_fft, rows, bins, 0) == 6
        assert _call(fft32, "kofft_hip_dev_mfcc_f32", r.addr, out, n_fft, rows, bins, nc) == 6
    assert _call(fft32, "kofft_hip_dev_mfcc_f32", r_out.addr + 4, r_out.addr, 1, 200, [0, 1, 2, 3, 4], 3) == 6
    arena.verify()
    assert_rows_equal(arena.read(r, F, (rows, n_fft)), x, "the refused calls left the input alone")
    assert _call(fft32, "kofft_hip_dev_mel_filterbank_f32", r.addr, r_out.addr, n_fft, rows, bins, 0) == 0
    arena.verify()
    assert_rows_equal(arena.read(r_out, F, (rows, 3)), mo.energies(x, bins), "one valid call after the refusals", nan_safe=True)
