"""visual::spectrogram's colour helpers on the device, every output byte against tests/spectrogram_oracle.py, every row checked.

Shapes: spec_image_kernel owns tiles of 64 bins x 64 frames and writes a picture row's run of frames as bytes up to the first 4-byte
boundary, whole dwords, then bytes; the row pitch frames * 3 (or * 6) is a multiple of 4 only for some frame counts, so the frame
counts sit one below, at and above a tile edge and give every phase of a row against the dwords.  spec_flat_kernel gives a lane four
consecutive pixels, so frames * bins takes every value mod 4.  Every case runs on the default context (the exchange through LDS) and on
one with kofft_hip_set_spectrogram_transpose(ctx, 0) (every lane stores its own bytes), through the device-pointer and the host-pointer
forms.  Kernel instances and the tests that launch them are listed in DESIGN.md 5.22."""
import ctypes as C

import numpy as np
import pytest

import spectrogram_oracle as so
from conftest import seeded
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32
BINS = [1, 2, 8, 16, 64, 512]
FRAMES = [1, 2, 3, 5, 63, 64, 65, 130]
MODES = [(0, -120.0), (1, 60.0)]


@pytest.fixture(scope="module")
def direct32():
    import kofft_amd
    from kofft_amd import spectrogram as sp

    f = kofft_amd.HipFftImpl(F)
    sp.set_transpose(False, fft=f)
    yield f
    f.close()


def _mags(frames, bins, seed):
    """Magnitudes spanning 1e-8 .. 1 times the maximum, the maximum itself and a value on the floor among them."""
    x = (F(1.75) * (10.0 ** seeded(seed).uniform(-8.0, 0.0, (frames, bins)))).astype(F)
    x.reshape(-1)[0] = F(1.75)
    if x.size > 1:
        x.reshape(-1)[-1] = F(1.75e-9)
    return x, F(1.75)


def _shape_as(want8, frames, depth, layout):
    """The oracle's frame-major 8-bit pixels of the first `frames` frames in another depth and layout."""
    w = want8[:frames]
    if depth == 16:
        w = w.astype(np.uint16) * np.uint16(257)
    if layout == 1:
        w = w[:, ::-1, :].transpose(1, 0, 2)
    return np.ascontiguousarray(w)


def _render(f, where, x, mx, mode, level, cmap, depth, scale, layout, table=None):
    from kofft_amd import spectrogram as sp

    if where == "host":
        return sp.render(x, mx, mode, level, cmap, depth, scale, layout, table, fft=f)
    import torch

    d_x = torch.from_numpy(x).cuda()
    d_m = torch.tensor([mx], dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    out = sp.render(d_x, d_m, mode, level, cmap, depth, scale, layout, table, fft=f)
    f.synchronize()
    got = out.cpu().numpy()
    return got.view(np.uint16) if depth == 16 else got


def _sweep(fft32, direct32, x_all, mx, bins, mode, level, scale, frames_list, what):
    for cmap in so.IMPLEMENTED:
        want8 = so.render(x_all, mx, mode, level, cmap, 8, scale, 0)  # once: a frame's pixels do not depend on the other frames
        for frames in frames_list:
            x = np.ascontiguousarray(x_all[:frames])
            for depth in (8, 16):
                for layout in (0, 1):
                    want = _shape_as(want8, frames, depth, layout)
                    tag = f"{what} cmap={cmap} frames={frames} depth={depth} layout={layout}"
                    assert_rows_equal(_render(fft32, "cuda", x, mx, mode, level, cmap, depth, scale, layout), want, tag + ": device form")
                    assert_rows_equal(_render(direct32, "host", x, mx, mode, level, cmap, depth, scale, layout), want,
                                      tag + ": host form, transpose off")


@pytest.mark.parametrize("scale", [0, 1])
@pytest.mark.parametrize("mode,level", MODES)
@pytest.mark.parametrize("bins", BINS)
def test_shapes(fft32, direct32, bins, mode, level, scale):
    x_all, mx = _mags(max(FRAMES), bins, 52000 + bins)
    _sweep(fft32, direct32, x_all, mx, bins, mode, level, scale, FRAMES, f"bins={bins} mode={mode} scale={scale}")


@pytest.mark.parametrize("bins,frames", [(1024, 67), (4096, 9)])
def test_long_frames(fft32, direct32, bins, frames):
    """Rows of 16 and 64 tiles; at 4096 bins the log map puts up to five bins on a pixel."""
    x_all, mx = _mags(frames, bins, 52100 + bins)
    _sweep(fft32, direct32, x_all, mx, bins, 0, -120.0, 1, [frames], f"bins={bins} log")
    _sweep(fft32, direct32, x_all, mx, bins, 1, 60.0, 0, [frames], f"bins={bins} linear")


def test_the_other_pairing_of_form_and_switch(fft32, direct32):
    """test_shapes pairs the device form with the LDS exchange and the host form with the direct stores: here the other way round."""
    x, mx = _mags(67, 70, 52200)
    for scale in (0, 1):
        want8 = so.render(x, mx, 0, -120.0, so.FIRE, 8, scale, 0)
        for depth in (8, 16):
            want = _shape_as(want8, 67, depth, 1)
            assert_rows_equal(_render(fft32, "host", x, mx, 0, -120.0, so.FIRE, depth, scale, 1), want, f"host form, LDS, depth={depth}")
            assert_rows_equal(_render(direct32, "cuda", x, mx, 0, -120.0, so.FIRE, depth, scale, 1), want, f"device form, direct, depth={depth}")


def test_every_palette_segment_and_both_ends_are_hit(fft32):
    """The seeded magnitudes reach the floor clamp, every segment of Fire and of Rainbow and both ends: no branch passes unseen."""
    x, mx = _mags(130, 64, 52064)
    for mode, level in MODES:
        t = so.color_t(x.reshape(-1), mx, mode, level)
        assert (t == 0).any() and (t == 1).any()
        fire, rainbow = so.fire_segment(so.clamp01(t)), so.rainbow_segment(so.clamp01(t))
        assert sorted(set(fire.tolist())) == [0, 1, 2, 3] and sorted(set(rainbow.tolist())) == [0, 1, 2, 3, 4]
        for cmap in so.IMPLEMENTED:
            assert_rows_equal(_render(fft32, "cuda", x, mx, mode, level, cmap, 8, 0, 0), so.render(x, mx, mode, level, cmap, 8, 0, 0),
                              f"mode={mode} cmap={cmap}")


def test_exact_segment_boundaries(fft32, direct32):
    """t = 0.25, 0.5, 0.75, 0.9 and 1 exactly: with max_mag 1 the magnitudes 10^-k have log10f = -k exactly, and the level puts them on
    the stops: 80 dB for 0.25 / 0.5 / 0.75 / 1, 200 dB for 0.9 -- checked on the oracle's t before the device is asked."""
    mags = (F(1.0) / np.array([10.0 ** k for k in range(8)], F)).astype(F)
    x = np.stack([mags, np.nextafter(mags, F(0.0)), np.nextafter(mags, F(2.0))]).astype(F)  # [3, 8]: on, below and above each stop
    hit = set()
    for mode, level in ((0, -80.0), (0, -200.0), (1, 80.0), (1, 200.0)):
        t = so.color_t(x[0], F(1.0), mode, level)
        hit |= {float(v) for v in t}
        for cmap in so.IMPLEMENTED:
            for layout in (0, 1):
                want = so.render(x, F(1.0), mode, level, cmap, 8, 0, layout)
                for f, where in ((fft32, "cuda"), (direct32, "host")):
                    assert_rows_equal(_render(f, where, x, F(1.0), mode, level, cmap, 8, 0, layout), want,
                                      f"mode={mode} level={level} cmap={cmap} layout={layout} {where}")
    assert {float(F(0.25)), 0.5, 0.75, float(F(0.9)), 1.0} <= hit, sorted(hit)


SPECIAL_MAGS = [0.0, -0.0, -1.0, np.nan, np.inf, 1e-45, 1e-39, 3.0, 1.0, 0.5, 1e-3, 1e-6, 1e-7, 2.5e-10, -np.inf, 0.999]


@pytest.mark.parametrize("max_mag", [1.0, 0.0, -1.0, float("nan"), 1e-40])
def test_special_values(fft32, direct32, max_mag):
    """mag 0, -1, NaN, +-inf, subnormal, above the maximum; max_mag 0, negative, NaN, subnormal; floors -120, -60, 0 and NaN; ranges 60
    and 120.  5 frames x 16 bins: every frame a rotation of the list, so every value meets every lane of a group of four."""
    x = np.stack([np.roll(np.array(SPECIAL_MAGS, F), r) for r in range(5)])
    mx = F(max_mag)
    for mode, level in ((0, -120.0), (0, -60.0), (0, 0.0), (0, float("nan")), (1, 60.0), (1, 120.0)):
        for cmap in so.IMPLEMENTED:
            for scale in (0, 1):
                want8 = so.render(x, mx, mode, level, cmap, 8, scale, 0)
                for depth, layout in ((8, 0), (8, 1), (16, 1)):
                    want = _shape_as(want8, 5, depth, layout)
                    for f, where in ((fft32, "cuda"), (direct32, "host")):
                        assert_rows_equal(_render(f, where, x, mx, mode, level, cmap, depth, scale, layout), want,
                                          f"max={max_mag} mode={mode} level={level} cmap={cmap} scale={scale} depth={depth} layout={layout} {where}")


@pytest.mark.parametrize("count", [1, 63, 64, 65, 100_003])
def test_pointwise(fft32, count):
    import torch
    from kofft_amd import spectrogram as sp

    x = (F(2.0) * (10.0 ** seeded(53000 + count).uniform(-9.0, 0.0, count))).astype(F)
    x[: min(count, len(SPECIAL_MAGS))] = np.array(SPECIAL_MAGS, F)[:count]
    for mx in (F(2.0), F(0.0), F(np.nan)):
        d_x, d_m = torch.from_numpy(x).cuda(), torch.tensor([mx], dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for level in (-120.0, -60.0, 0.0, float("nan")):
            want = so.magnitude_to_db(x, mx, level)
            assert_rows_equal(sp.magnitude_to_db(x, mx, level, fft=fft32), want, f"magnitude_to_db host count={count} max={mx} floor={level}", nan_safe=True)
            got = sp.magnitude_to_db(d_x, d_m, level, fft=fft32)
            fft32.synchronize()
            assert_rows_equal(got.cpu().numpy(), want, f"magnitude_to_db device count={count} max={mx} floor={level}", nan_safe=True)
        for level in (60.0, 120.0):
            want = so.db_scale(x, mx, level)
            assert_rows_equal(sp.db_scale(x, mx, level, fft=fft32), want, f"db_scale host count={count} max={mx} range={level}", nan_safe=True)
            got = sp.db_scale(d_x, d_m, level, fft=fft32)
            fft32.synchronize()
            assert_rows_equal(got.cpu().numpy(), want, f"db_scale device count={count} max={mx} range={level}", nan_safe=True)


def test_magnitudes_to_picture_without_leaving_the_device(fft32, oracle):
    """kofft_hip_dev_stft_magnitudes_rows_f32 (win 64, hop 32, 4096 samples) -> render with that call's d_max, against the two oracles
    composed."""
    import torch
    from kofft_amd import spectrogram as sp

    sig = seeded(54000).uniform(-1.0, 1.0, 4096).astype(F)
    frames, bins = 128, 32
    d_sig = torch.from_numpy(sig).cuda()
    d_mags = torch.zeros((frames, bins), dtype=torch.float32, device="cuda")
    d_max = torch.zeros(1, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    fft32.stft_magnitudes_rows_dev(d_sig.data_ptr(), 1, 4096, 4096, 64, 32, d_mags.data_ptr(), frames, d_max.data_ptr())
    pic = sp.render(d_mags, d_max, 0, -120.0, "fire", 8, "log", "image", fft=fft32)
    pic16 = sp.render(d_mags, d_max, 1, 80.0, "rainbow", 16, "linear", "image", fft=fft32)
    fft32.synchronize()
    mags, mx = oracle.stft_magnitudes(sig, 64, 32)
    assert mags.shape == (frames, bins)
    assert_rows_equal(pic.cpu().numpy(), so.render(mags, mx, 0, -120.0, so.FIRE, 8, 1, 1), "magnitudes -> log-scaled Fire picture")
    assert_rows_equal(pic16.cpu().numpy().view(np.uint16), so.render(mags, mx, 1, 80.0, so.RAINBOW, 16, 0, 1), "magnitudes -> Rainbow u16 picture")


def test_a_callers_own_table(fft32, direct32):
    """The table is an input: empty pixels, one pixel holding most of the row, and the cache of four tables turning over."""
    bins, frames = 70, 66
    x, mx = _mags(frames, bins, 55000)
    tables = [np.minimum(np.arange(bins) // k, bins - 1).astype(np.uint32) for k in (1, 2, 3, 7, 70)] + [np.full(bins, bins - 1, np.uint32)]
    tables.append(np.concatenate([np.zeros(60, np.uint32), np.arange(60, 70, dtype=np.uint32)]))
    for rnd in range(2):
        for i, t in enumerate(tables):
            want = so.render(x, mx, 0, -120.0, so.GRAY, 8, 1, 1, table=t)
            assert_rows_equal(_render(fft32, "cuda", x, mx, 0, -120.0, so.GRAY, 8, 1, 1, t), want, f"table {i} round {rnd}")
            assert_rows_equal(_render(direct32, "host", x, mx, 0, -120.0, so.GRAY, 8, 1, 0, t),
                              so.render(x, mx, 0, -120.0, so.GRAY, 8, 1, 0, table=t), f"table {i} round {rnd} frame-major")


def _raw(f, name, mags, frames, bins, mx, out, mode=0, level=-120.0, cmap=0, depth=8, scale=0, layout=0, table=None):
    t = None if table is None else C.c_void_p(np.ascontiguousarray(table, np.uint32).ctypes.data)
    return getattr(f._lib, name)(f._ctx, C.c_void_p(mags), frames, bins, C.c_void_p(mx), mode, level, cmap, depth, scale, layout, t, C.c_void_p(out))


def test_errors_then_a_valid_call(fft32):
    """Every refusal of include/kofft_hip.h on a live context, the overlap refusals of the device forms, then one valid call."""
    import torch

    frames, bins = 6, 8
    x, mx = _mags(frames, bins, 56000)
    d_x, d_m = torch.from_numpy(x).cuda(), torch.tensor([mx], dtype=torch.float32, device="cuda")
    d_out = torch.zeros(frames * bins * 6, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dev, host = "kofft_hip_dev_spectrogram_render_f32", "kofft_hip_spectrogram_render_f32"
    a, m, o = d_x.data_ptr(), d_m.data_ptr(), d_out.data_ptr()
    assert _raw(fft32, dev, a, 0, bins, m, o) == 1 and _raw(fft32, dev, a, frames, 0, m, o) == 1
    for kw in ({"mode": 2}, {"cmap": 3}, {"cmap": 4}, {"cmap": 5}, {"cmap": 7}, {"depth": 12}, {"scale": 2}, {"layout": 2}):
        assert _raw(fft32, dev, a, frames, bins, m, o, **kw) == 6, kw
    assert _raw(fft32, dev, a, frames, bins, m, o, scale=1) == 6
    assert _raw(fft32, dev, a, frames, bins, m, o, scale=1, table=[0, 1, 2, 3, 4, 5, 6, 8]) == 6
    assert _raw(fft32, dev, a, frames, bins, m, o, scale=1, table=[0, 1, 3, 2, 4, 5, 6, 7]) == 6
    assert _raw(fft32, dev, 0, frames, bins, m, o) == -3 and _raw(fft32, dev, a, frames, bins, 0, o) == -3 and _raw(fft32, dev, a, frames, bins, m, 0) == -3
    # the output over the input (its start, its last byte), the input inside the output, the output over max_mag
    nb = frames * bins * 4
    assert _raw(fft32, dev, a, frames, bins, m, a) == 6 and _raw(fft32, dev, a, frames, bins, m, a + nb - 1) == 6
    assert _raw(fft32, dev, o + 4, 1, 2, m, o) == 6 and _raw(fft32, dev, a, frames, bins, o + 4, o) == 6
    for name in ("kofft_hip_dev_magnitude_to_db_f32", "kofft_hip_dev_db_scale_f32"):
        fn = getattr(fft32._lib, name)
        assert fn(fft32._ctx, C.c_void_p(a), 0, C.c_void_p(m), -120.0, C.c_void_p(o)) == 1
        assert fn(fft32._ctx, C.c_void_p(a), 8, C.c_void_p(m), -120.0, C.c_void_p(a + 4)) == 6
        assert fn(fft32._ctx, C.c_void_p(a), 8, C.c_void_p(o + 8), -120.0, C.c_void_p(o)) == 6
        assert fn(fft32._ctx, None, 8, C.c_void_p(m), -120.0, C.c_void_p(o)) == -3
    fft32.synchronize()
    assert np.array_equal(d_x.cpu().numpy(), x) and not d_out.cpu().numpy().any(), "a refused call wrote something"
    hx, hm, ho = x.copy(), np.array([mx], F), np.zeros(frames * bins * 3, np.uint8)
    assert _raw(fft32, host, hx.ctypes.data, frames, bins, hm.ctypes.data, ho.ctypes.data, cmap=4) == 6 and not ho.any()
    assert _raw(fft32, dev, a, frames, bins, m, o, layout=1, depth=16, cmap=6) == 0
    fft32.synchronize()
    got = d_out.cpu().numpy().view(np.uint16).reshape(bins, frames, 3)
    assert_rows_equal(got, so.render(x, mx, 0, -120.0, so.RAINBOW, 16, 0, 1), "one valid call after the refusals")


def test_contexts_streams_and_released_scratch(fft32):
    """A second context, another stream, and kofft_hip_release_scratch between calls (it drops the cached pixel ranges)."""
    import kofft_amd
    import torch
    from kofft_amd import spectrogram as sp

    x, mx = _mags(65, 40, 57000)
    want = so.render(x, mx, 0, -120.0, so.FIRE, 8, 1, 1)
    other = kofft_amd.HipFftImpl(F)
    try:
        for f in (fft32, other, fft32):
            assert_rows_equal(_render(f, "cuda", x, mx, 0, -120.0, so.FIRE, 8, 1, 1), want, "two contexts")
        assert other._lib.kofft_hip_release_scratch(other._ctx) == 0
        assert_rows_equal(_render(other, "cuda", x, mx, 0, -120.0, so.FIRE, 8, 1, 1), want, "after release_scratch")
        assert_rows_equal(_render(other, "host", x, mx, 0, -120.0, so.FIRE, 8, 1, 1), want, "after release_scratch, host form")
        stream = torch.cuda.Stream()
        other.set_stream(stream.cuda_stream)
        d_x, d_m = torch.from_numpy(x).cuda(), torch.tensor([mx], dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        out = sp.render(d_x, d_m, 0, -120.0, "fire", 8, "log", "image", fft=other)
        stream.synchronize()
        assert_rows_equal(out.cpu().numpy(), want, "on a caller's stream")
        other.set_stream(0)
    finally:
        other.close()
