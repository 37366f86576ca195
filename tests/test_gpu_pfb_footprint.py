"""Guard bands (tests/redzone.py) around every buffer of the polyphase filter-bank entries, device-pointer and
host-pointer forms: a call writes its output and nothing else, leaves x, h, g and spec as they were, and the result inside the bands is
the oracle's.

Cases, all at bins < M (the one-sided form, and a shorter prefix for the analysis): ragged last workgroups of the fused kernels, rows a
stride apart (the gaps are band pattern: a NaN, so a read of a neighbour's gap shows in the result), leads 0 and nh - 1, frames past the
row's end, windows of the synthesis that start and end inside a hop block, real buffers that are only 4-byte aligned, lengths only the
composed route takes, every route of the rest."""
import ctypes as C

import numpy as np
import pytest

from conftest import seeded
import pfb_oracle as po
from redzone import Arena
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def routes(fft32):
    """the default context, the composed route alone (set_pfb_fused(False)) and the fused kernels wherever they exist (set_pfb_fused(2))"""
    import kofft_amd

    composed, forced = kofft_amd.HipFftImpl(F), kofft_amd.HipFftImpl(F)
    composed.set_pfb_fused(False)
    forced.set_pfb_fused(2)
    yield ((fft32, "default"), (composed, "composed"), (forced, "fused"))
    composed.close()
    forced.close()


# (M, T, D, rows, nx, row stride, lead, frames, bins, offsets of x and h / out in bytes; out is complex: 8-byte aligned)
ANALYSIS_CASES = [(64, 4, 64, 7, 700, 700, 0, 13, 33, 0, 0), (64, 3, 29, 5, 333, 340, 191, 20, 5, 4, 8), (1024, 2, 512, 3, 5000, 5001, 1536, 15, 513, 4, 8),
                  (4096, 2, 4103, 2, 20000, 20010, 4096, 7, 2049, 0, 8), (2, 3, 1, 5, 9, 11, 5, 17, 1, 4, 0), (240, 3, 100, 3, 1500, 1503, 620, 23, 121, 0, 0),
                  (8192, 2, 8192, 2, 40000, 40000, 8192, 7, 4097, 0, 0)]


@pytest.mark.parametrize("m,taps,hop,rows,nx,stride,lead,frames,bins,off_in,off_out", ANALYSIS_CASES)
@pytest.mark.parametrize("where", ["cuda", "host"])
def test_analysis_guard_bands(routes, where, m, taps, hop, rows, nx, stride, lead, frames, bins, off_in, off_out):
    rng = seeded(16500 + m + nx)
    nh = taps * m
    x = rng.uniform(-1, 1, (rows, nx)).astype(F)
    h = rng.uniform(0.1, 1, nh).astype(F)
    want = po.analysis_ref(x, h, m, hop, lead, frames, bins).reshape(rows, frames * bins)
    name = "kofft_hip_dev_pfb_analysis_f32" if where == "cuda" else "kofft_hip_pfb_analysis_f32"
    for f, route in routes:
        arena = Arena(where, f"{name} M={m} T={taps} D={hop} rows={rows} nx={nx} stride={stride} lead={lead} frames={frames} bins={bins} {route}")
        # the gaps between the rows hold NaN and are part of the input region: never written, and not read either (the result)
        padded = np.full((rows, stride), np.nan, F)
        padded[:, :nx] = x
        r_x = arena.input(padded.reshape(-1)[:(rows - 1) * stride + nx], align_off=off_in, row_bytes=4 * stride)
        r_h = arena.input(h, align_off=off_in)
        r_out = arena.output(8 * frames * bins * rows, align_off=off_out, row_bytes=8 * frames * bins)
        for _ in range(2):
            rc = getattr(f._lib, name)(f._ctx, C.c_void_p(r_x.addr), rows, nx, stride, C.c_void_p(r_h.addr), nh, m, hop, lead, C.c_void_p(r_out.addr),
                                       frames, bins)
            assert rc == 0, arena.what
        arena.verify()
        assert_rows_equal(arena.read(r_out, np.complex64, (rows, frames * bins)), want, arena.what)


# (M, T, D, rows, frames, out_first, out_len (None: to the end), offsets of spec / g and out in bytes); bins = M / 2 + 1
SYNTHESIS_CASES = [(64, 4, 64, 7, 5, 0, None, 0, 0, 0), (64, 3, 29, 5, 9, 64, 300, 8, 4, 12), (1024, 2, 512, 3, 6, 1500, 2049, 8, 4, 4),
                   (4096, 2, 4093, 2, 3, 100, 50, 0, 0, 4), (2, 3, 1, 5, 7, 3, 9, 8, 4, 0), (240, 3, 100, 3, 6, 240, 900, 0, 0, 0),
                   (8192, 2, 8192, 2, 3, 8192, 16384, 0, 0, 0)]


@pytest.mark.parametrize("m,taps,hop,rows,frames,first,count,off_spec,off_g,off_out", SYNTHESIS_CASES)
@pytest.mark.parametrize("where", ["cuda", "host"])
def test_synthesis_guard_bands(routes, where, m, taps, hop, rows, frames, first, count, off_spec, off_g, off_out):
    rng = seeded(16600 + m + frames)
    nh, bins = taps * m, m // 2 + 1
    S = (rng.uniform(-1, 1, (rows, frames, bins)) + 1j * rng.uniform(-1, 1, (rows, frames, bins))).astype(np.complex64)
    g = rng.uniform(0.1, 1, nh).astype(F)
    full = (frames - 1) * hop + nh
    count = full - first if count is None else count
    scale = F(0.75)
    want = np.ascontiguousarray(po.synthesis_ref(S, g, m, hop, scale)[:, first:first + count])
    name = "kofft_hip_dev_pfb_synthesis_f32" if where == "cuda" else "kofft_hip_pfb_synthesis_f32"
    for f, route in routes:
        arena = Arena(where, f"{name} M={m} T={taps} D={hop} rows={rows} frames={frames} window=({first}, {count}) {route}")
        r_S = arena.input(S, align_off=off_spec, row_bytes=8 * frames * bins)
        r_g = arena.input(g, align_off=off_g)
        r_out = arena.output(4 * count * rows, align_off=off_out, row_bytes=4 * count)
        for _ in range(2):
            rc = getattr(f._lib, name)(f._ctx, C.c_void_p(r_S.addr), rows, frames, bins, C.c_void_p(r_g.addr), nh, m, hop, C.c_float(float(scale)),
                                       C.c_void_p(r_out.addr), first, count)
            assert rc == 0, arena.what
        arena.verify()
        assert_rows_equal(arena.read(r_out, F, (rows, count)), want, arena.what)
