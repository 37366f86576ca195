"""Audio -> spectrogram pictures in one call (kofft_hip_stft_picture_f32 and its kofft_hip_dev_ form) against the existing oracles
composed (tests/picture_oracle.py: the front end's magnitudes, the row / running / given maximum, the render's colours): every picture
row of every row of the batch byte for byte (tests/rowcheck.py), and max_out bit for bit.

Shapes are the smallest that cross each edge: the render's 64 x 64 tile, the STFT kernels' frames per workgroup, row seams, chunk seams
inside a row (KOFFT_HIP_SCRATCH_CHUNK_MB=1 around a context of the test's own), a wavefront and a workgroup of bins for the running
maximum.  The option space (2 layouts x 3 pixel formats x 2 scales x 2 colour modes x 4 palettes x 3 maximum modes x host / device form)
is walked as a covering rotation, not a product: case i of a test takes layout i % 2, pixel format (i // 2) % 3, scale (i // 3) % 2,
colour mode (i // 4) % 2, palette i % 4, maximum mode i % 3 and the host form when (i // 2) % 2 -- every value of every option, and every
pair (layout, format), (format, maximum mode), (scale, mode) occurs within 12 consecutive cases.  Kernel instances and the tests that
launch them are listed in DESIGN.md 5.24."""
import ctypes as C

import numpy as np
import pytest

import frontend_oracle as fo
import picture_oracle as po
import spectrogram_oracle as so
from conftest import bits_equal, seeded
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32
KNOB = "KOFFT_HIP_SCRATCH_CHUNK_MB"
FORMATS = [(8, 3), (8, 4), (16, 3)]
PALETTES = [so.FIRE, so.LEGACY, so.GRAY, so.RAINBOW]
XPB = {64: 16, 128: 16, 256: 16, 512: 4, 1024: 4, 2048: 2}  # the generic STFT kernel's frames per workgroup


def options(i):
    """The covering rotation of the module docstring: (kw for the oracle and the call, host form?)."""
    depth, channels = FORMATS[(i // 2) % 3]
    kw = dict(max_mode=i % 3, mode=(i // 4) % 2, level=[-80.0, 60.0][(i // 4) % 2], cmap=PALETTES[i % 4], depth=depth, channels=channels,
              scale=(i // 3) % 2, layout=i % 2)
    if kw["max_mode"] == 1:
        kw["scale"] = 0
    return kw, bool((i // 2) % 2)


def shape_of(rows, frames, bins, layout, channels):
    return (rows, frames, bins, channels) if layout == 0 else (rows, bins, frames, channels)


def run_dev(f, x, win_len, hop, frames, window=None, max_in=None, table=None, want_max=True, **kw):
    """The device form on fresh buffers pre-filled with a pattern: (pictures, max_out)."""
    import torch

    rows, length = x.shape
    bins = win_len // 2
    dt = np.uint16 if kw["depth"] == 16 else np.uint8
    shape = shape_of(rows, frames, bins, kw["layout"], kw["channels"])
    nbytes = int(np.prod(shape)) * np.dtype(dt).itemsize
    d_x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_w = torch.from_numpy(np.ascontiguousarray(window, F)).cuda() if window is not None else None
    d_in = torch.from_numpy(np.ascontiguousarray(max_in, F)).cuda() if max_in is not None else None
    d_out = torch.full((nbytes + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    d_max = torch.full((rows,), float("nan"), device="cuda")
    torch.cuda.synchronize()
    f.stft_picture_rows_dev(d_x.data_ptr() if length else 0, rows, length, length, d_w.data_ptr() if d_w is not None else 0, win_len, hop, frames,
                            kw["max_mode"], d_in.data_ptr() if d_in is not None else 0, d_max.data_ptr() if want_max else 0, kw["mode"], kw["level"],
                            kw["cmap"], kw["depth"], kw["channels"], kw["scale"], kw["layout"], table, d_out.data_ptr())
    f.synchronize()
    raw = d_out.cpu().numpy()
    assert (raw[nbytes:] == 0xA5).all(), "bytes past the pictures"
    return raw[:nbytes].view(dt).reshape(shape), d_max.cpu().numpy()


def run_host(f, x, win_len, hop, frames, window=None, max_in=None, table=None, **kw):
    return f.stft_picture_rows(x, win_len, hop, window, frames, kw["max_mode"], max_in, kw["mode"], kw["level"], kw["cmap"], kw["depth"],
                               kw["channels"], kw["scale"], kw["layout"], table)


def assert_pictures(got, want, what):
    """every picture row of every picture"""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    width = got.shape[-2] * got.shape[-1]
    assert_rows_equal(got.reshape(-1, width), want.reshape(-1, width), what)


def check(f, oracle, x, win_len, hop, frames, kw, host, what, window=None, max_in=None):
    table = so.log_bin_map(win_len // 2) if kw["scale"] == 1 else None
    if kw["max_mode"] == 2 and max_in is None:
        max_in = np.linspace(0.5, 40.0, x.shape[0]).astype(F)
    want, want_max, mags = po.expected(oracle, x, win_len, hop, frames, window, max_in=max_in, table=table, **kw)
    run = run_host if host else run_dev
    got, got_max = run(f, x, win_len, hop, frames, window=window, max_in=max_in, table=table, **kw)
    what = f"{what} {'host' if host else 'dev'} {kw}"
    assert_pictures(got, want, what)
    assert bits_equal(got_max, want_max), (what, got_max, want_max)
    return got, got_max, mags


@pytest.mark.parametrize("win_len", [32, 64, 256, 1024, 4096])
def test_tile_edges(fft32, oracle, win_len):
    """frames one below, at and one above the render's 64-frame tile and the STFT kernel's frames per workgroup, rows 1 .. 3 (the flat
    index crosses row seams inside a workgroup and a chunk of one piece holds several rows), hops of 1 (len < win_len: every frame is
    partly zeros), win_len / 4, win_len and win_len + 3; the options by the rotation of the module docstring."""
    tile = XPB.get(win_len, 4)
    mult = tile if tile >= 8 else 2 * tile
    i = win_len  # (another start of the rotation per window length)
    for hop in (1, win_len // 4, win_len, win_len + 3):
        for frames in (mult - 1, mult, mult + 1, 63, 64, 65):
            rows = 1 + i % 3
            kw, host = options(i)
            i += 1
            length = frames * hop - hop // 2
            assert -(-length // hop) == frames
            x = fo.signal(seeded(61000 + win_len + i), rows, length)
            check(fft32, oracle, x, win_len, hop, frames, kw, host, f"win_len={win_len} hop={hop} rows={rows} frames={frames}")


@pytest.mark.parametrize("win_len,hop,length", [(256, 64, 1000), (1024, 256, 700), (64, 64, 10)])
def test_more_frames_than_the_signal_fills(fft32, oracle, win_len, hop, length):
    """frames two more than ceil(len / hop): the extra frames are silence, coloured as +0 against the row's maximum; a row shorter than
    the window."""
    frames = -(-length // hop) + 2
    x = fo.signal(seeded(62000 + win_len), 3, length, special=False)
    for i in range(6):
        kw, host = options(i)
        _, _, mags = check(fft32, oracle, x, win_len, hop, frames, kw, host, f"win_len={win_len} frames={frames}")
    assert bits_equal(mags[:, -2:], np.zeros((3, 2, win_len // 2), F)), "the oracle's silence"


@pytest.mark.parametrize("win_len,hop", [(256, 64), (400, 150)])
def test_a_callers_window_and_a_bluestein_length(fft32, oracle, win_len, hop):
    from kofft_amd import window

    rows, frames = 2, 21
    x = fo.signal(seeded(63000 + win_len), rows, frames * hop - 11)
    for i in range(6):
        kw, host = options(i)
        check(fft32, oracle, x, win_len, hop, frames, kw, host, f"hamming({win_len})", window=window.hamming(win_len))


@pytest.fixture(scope="module")
def seam_case(oracle):
    """3 rows of 153 700 samples, win 1024, hop 256: 601 frames per row; the magnitudes once for every mode."""
    x = fo.signal(seeded(64000), 3, 153700)
    return x, fo.magnitudes(oracle, x, 1024, 256, 601)


@pytest.mark.parametrize("max_mode", [0, 1, 2])
def test_chunk_seams_inside_a_row(monkeypatch, seam_case, max_mode):
    """KOFFT_HIP_SCRATCH_CHUNK_MB=1: 1803 frames of 2 KiB of magnitudes are 512 per chunk (modes 0 and 2; the running maximum keeps a
    second array and takes 256), so chunks begin at (row 0, frame 512), (row 1, frame 423) and (row 2, frame 334): one on the render's
    64-frame tile and two not, and the picture's pitch is 1803 bytes, odd.  Mode 0 cannot keep the magnitudes, so its maximum comes from
    the max-only pass of the magnitudes kernels (the generic one at this batch).  Both layouts, the LDS transpose on and off."""
    import kofft_amd

    win_len, hop, frames, rows = 1024, 256, 601, 3
    assert -(-153700 // hop) == frames and frames * 3 == 1803 and (1 << 20) // (4 * 512) == 512
    assert [divmod(t, frames) for t in range(512, rows * frames, 512)] == [(0, 512), (1, 423), (2, 334)]
    assert 512 % 64 == 0 and 423 % 64 and 334 % 64 and (frames * 3) % 4 == 3
    assert [divmod(t, frames) for t in range(256, rows * frames, 256)][:3] == [(0, 256), (0, 512), (1, 167)]  # the running maximum's seams
    x, mags = seam_case
    monkeypatch.setenv(KNOB, "1")
    f = kofft_amd.HipFftImpl(F)
    try:
        max_in = np.array([3.0, 0.25, 700.0], F)
        for layout in (0, 1):
            kw = dict(max_mode=max_mode, mode=0, level=-80.0, cmap=so.RAINBOW, depth=8, channels=3, scale=0, layout=layout)
            want, want_max = po.pictures(mags, max_in=max_in, **kw)
            for transpose in (True, False):
                f._check(f._lib.kofft_hip_set_spectrogram_transpose(f._ctx, int(transpose)))
                got, got_max = run_dev(f, x, win_len, hop, frames, max_in=max_in if max_mode == 2 else None, **kw)
                assert_pictures(got, want, f"seams: max_mode {max_mode} layout {layout} transpose {transpose}")
                assert bits_equal(got_max, want_max), (max_mode, layout, got_max, want_max)
        for depth, channels in ((8, 4), (16, 3)):  # the other two pixel formats in the image layout, a pitch of 2404 and of 3606 bytes
            kw = dict(max_mode=max_mode, mode=1, level=70.0, cmap=so.FIRE, depth=depth, channels=channels, scale=0, layout=1)
            want, want_max = po.pictures(mags, max_in=max_in, **kw)
            for transpose in (True, False):
                f._check(f._lib.kofft_hip_set_spectrogram_transpose(f._ctx, int(transpose)))
                got, got_max = run_dev(f, x, win_len, hop, frames, max_in=max_in if max_mode == 2 else None, **kw)
                assert_pictures(got, want, f"seams: max_mode {max_mode} depth {depth} channels {channels} image, transpose {transpose}")
                assert bits_equal(got_max, want_max)
    finally:
        f.close()


# (win_len, hop, rows, frames): with a 1 MiB chunk the magnitudes take at least two chunks, and the batch reaches the named family of the
# magnitudes kernels on a device of 256 compute units (dispatch(), host_common.hip.h)
MAX_ONLY = {"small n=2": (2, 1, 2, 140000), "small n=16": (16, 3, 2, 20000), "small n=32": (32, 8, 3, 8000), "generic n=256": (256, 64, 2, 1500),
            "generic n=4096": (4096, 1024, 2, 80), "generic n=16384": (16384, 4096, 1, 40), "persistent n=256": (256, 4, 2, 16400),
            "persistent n=1024": (1024, 16, 1, 8300), "persistent n=4096": (4096, 64, 1, 1100), "composed n=400": (400, 150, 2, 400)}


@pytest.mark.parametrize("family", sorted(MAX_ONLY))
def test_the_max_only_pass_on_every_kernel_family(monkeypatch, oracle, family):
    """Mode 0 over more than one chunk: the maxima come from the magnitudes kernels without their stores (StftMagRowsMaxOnlyIO; a
    composed window length: from the chunks in scratch).  max_out against the oracle's row maximum bit for bit; the pictures against
    the same context's mode 2 fed that maximum (which the other tests hold to the oracle) -- the pass under test only chooses the maximum."""
    import kofft_amd

    win_len, hop, rows, frames = MAX_ONLY[family]
    length = frames * hop - hop // 2
    per_frame = (win_len // 2) * 4 + (0 if win_len & (win_len - 1) == 0 else win_len * 8)  # (a composed length keeps its frames there too)
    assert -(-length // hop) == frames and rows * frames * per_frame > 1 << 20, "more than one chunk"
    x = fo.signal(seeded(65000 + win_len), rows, length)
    mags = fo.magnitudes(oracle, x, win_len, hop, frames)
    want_max = np.array([po.row_max(mags[r]) for r in range(rows)], F)
    kw = dict(mode=0, level=-80.0, cmap=so.LEGACY, depth=8, channels=3, scale=0, layout=1)
    monkeypatch.setenv(KNOB, "1")
    f = kofft_amd.HipFftImpl(F)
    try:
        got, got_max = run_dev(f, x, win_len, hop, frames, max_mode=0, **kw)
        assert bits_equal(got_max, want_max), (family, got_max, want_max)
        given, _ = run_dev(f, x, win_len, hop, frames, max_in=want_max, max_mode=2, **kw)
        assert_pictures(got, given, family)
        r = rows - 1  # one picture against the oracle as well, where that is small
        if frames * (win_len // 2) <= 1 << 18:
            want, _ = po.pictures(mags[r:r + 1], max_mode=0, **kw)
            assert_pictures(got[r:r + 1], want, family + ": the oracle")
    finally:
        f.close()


class ComputeFrame:
    """web-spectrogram's State::compute_frame (src/lib.rs:211-234) restated: the buffer, the window product, the transform, and per bin
    `if mag > max_mag { max_mag = mag }` BEFORE color_from_magnitude_u8(mag, max_mag, FLOOR_DB, Rainbow), pixels R, G, B, 255."""

    def __init__(self, oracle, win_len, hop, floor_db=-80.0):
        self.oracle, self.win_len, self.hop, self.floor = oracle, win_len, hop, floor_db
        self.window = oracle.hann(win_len)
        self.buf = np.zeros(0, F)
        self.max_mag = F(1e-12)

    def feed(self, samples):
        self.buf = np.concatenate([self.buf, np.asarray(samples, F)])
        if self.buf.size < self.win_len:
            return np.zeros(0, np.uint8)
        st = self.oracle.stft(np.ascontiguousarray(self.buf[:self.win_len]), self.window, self.win_len, 1)[0, :self.win_len // 2]
        re, im = np.ascontiguousarray(st.real, F), np.ascontiguousarray(st.imag, F)
        with np.errstate(all="ignore"):
            mags = np.sqrt(re * re + im * im)
        used, mx = [], float(self.max_mag)  # (f32 values as Python floats: the same order)
        for mag in mags.tolist():
            if mag > mx:
                mx = mag
            used.append(mx)
        used, self.max_mag = np.array(used, F), F(mx)
        row = po.with_alpha(po.render_elem(mags[None], used[None], 0, self.floor, so.RAINBOW, 8, 0), 4)
        self.buf = self.buf[self.hop:]
        return row.reshape(-1)


# win_len: (hop, frames per row): a frame is 1, 16, 32, 128, 512 or 2048 bins; with a 1 MiB chunk and the second array the 4 rows cross a seam
RUNNING = {2: (1, 40000), 32: (8, 2500), 64: (16, 1200), 256: (64, 300), 1024: (256, 601), 4096: (1024, 43)}


@pytest.mark.parametrize("win_len", sorted(RUNNING))
def test_the_running_maximum(monkeypatch, oracle, win_len):
    """Row 0: N(0, 1) under an amplitude ramp 1 .. 100 (the maximum keeps moving, between frames and inside them); row 1: the loudest
    frame first (it never moves again); row 2: a NaN sample, row 3: an inf sample, each poisoning exactly the frames that cover it.
    KOFFT_HIP_SCRATCH_CHUNK_MB=1: the carry survives a chunk seam and starts again at a row start inside a chunk.  Then the frames that
    lie wholly inside the signal against compute_frame restated, fed win_len samples, then hop at a time."""
    import kofft_amd

    hop, frames = RUNNING[win_len]
    bins, rows = win_len // 2, 4
    length = frames * hop - hop // 2
    assert -(-length // hop) == frames
    per_chunk = (1 << 20) // (8 * bins)
    assert rows * frames > per_chunk and per_chunk % frames, "a seam, and not at a row start"
    rng = seeded(66000 + win_len)
    x = rng.standard_normal((rows, length)).astype(F)
    x[0] *= (1 + 99 * np.arange(length) / length).astype(F)
    x[1, :hop] *= F(1e4)  # (only frame 0 covers these samples)
    x[2, length // 2] = np.nan
    x[3, length // 3] = np.inf
    kw = dict(max_mode=1, mode=0, level=-80.0, cmap=so.RAINBOW, depth=8, channels=4, scale=0, layout=0)
    want, want_max, mags = po.expected(oracle, x, win_len, hop, frames, **kw)
    pm = po.running_max(mags[0])
    if win_len >= 32:
        moved = pm.reshape(-1)[1:] > pm.reshape(-1)[:-1]
        at_frame, at_bin = np.divmod(np.flatnonzero(moved) + 1, bins)
        assert len(set(at_frame)) >= 10 and (at_bin > 0).sum() >= 10, "the ramp moves the maximum between frames and inside them"
        p1 = po.running_max(mags[1])
        assert (p1[1:] == p1[0, -1]).all(), "row 1: the loudest frame is the first"
        assert np.isfinite(want_max[:3]).all()
    hit = [k for k in range(frames) if k * hop <= length // 3 < k * hop + win_len]
    assert not np.isfinite(mags[3][hit]).all(axis=1).any() and np.isfinite(np.delete(mags[3], hit, axis=0)).all(), "row 3: the inf poisons exactly the frames that cover it"
    assert np.isnan(mags[2]).any() and not np.isnan(po.running_max(mags[2])).any()
    monkeypatch.setenv(KNOB, "1")
    f = kofft_amd.HipFftImpl(F)
    try:
        got, got_max = run_dev(f, x, win_len, hop, frames, **kw)
        assert_pictures(got, want, f"running maximum, win_len {win_len}, frames layout RGBA")
        assert bits_equal(got_max, want_max), (got_max, want_max)
        kw2 = dict(kw, layout=1, channels=3, mode=1, level=90.0, cmap=so.FIRE)
        want2, _ = po.pictures(mags, **kw2)
        got2, _ = run_dev(f, x, win_len, hop, frames, want_max=False, **kw2)
        assert_pictures(got2, want2, f"running maximum, win_len {win_len}, image layout")
    finally:
        f.close()
    # compute_frame, literally, from the start of row 0: every frame that lies inside the signal (win_len 2: the first 3000 of the
    # 40 000 one-bin frames, which would take most of a minute of scalar Python)
    whole = (length - win_len) // hop + 1
    n = whole if win_len > 2 else 3000
    cf = ComputeFrame(oracle, win_len, hop)
    lines = [cf.feed(x[0, :win_len])] + [cf.feed(x[0, win_len + (k - 1) * hop: win_len + k * hop]) for k in range(1, n)]
    assert all(line.size == bins * 4 for line in lines)
    assert_rows_equal(got[0, :n].reshape(n, -1), np.stack(lines), f"compute_frame restated, win_len {win_len}")


def test_equalities_with_the_two_call_chain(fft32, oracle):
    """Mode 0, Hann, frames == ceil(len / hop): the bytes of stft_magnitudes_rows_dev -> spectrogram_render_dev per row on the same
    context, max_out the chain's d_max bit for bit; mode 2 fed mode 0's max_out reproduces mode 0; channels 4 without alpha is channels 3."""
    import torch

    rows, length, win_len, hop = 3, 2048, 256, 64
    frames, bins = length // hop, win_len // 2
    x = seeded(67000).uniform(-1, 1, (rows, length)).astype(F)
    d_sig = torch.from_numpy(x).cuda()
    d_mags = torch.full((rows, frames, bins), float("nan"), device="cuda")
    d_max = torch.full((rows,), float("nan"), device="cuda")
    torch.cuda.synchronize()
    fft32.stft_magnitudes_rows_dev(d_sig.data_ptr(), rows, length, length, win_len, hop, d_mags.data_ptr(), frames, d_max.data_ptr())
    for layout in (0, 1):
        for depth in (8, 16):
            kw = dict(mode=0, level=-100.0, cmap=so.FIRE, depth=depth, channels=3, scale=0, layout=layout)
            px = 3 * depth // 8
            chain = torch.full((rows, frames * bins * px), 0x5A, dtype=torch.uint8, device="cuda")
            for r in range(rows):
                fft32._check(fft32._lib.kofft_hip_dev_spectrogram_render_f32(fft32._ctx, C.c_void_p(d_mags[r].data_ptr()), frames, bins,
                                                                             C.c_void_p(d_max[r].data_ptr()), 0, -100.0, so.FIRE, depth, 0, layout,
                                                                             None, C.c_void_p(chain[r].data_ptr())))
            fft32.synchronize()
            one, mx = run_dev(fft32, x, win_len, hop, frames, max_mode=0, **kw)
            assert one.tobytes() == chain.cpu().numpy().tobytes(), (layout, depth)
            assert bits_equal(mx, d_max.cpu().numpy())
            given, mx2 = run_dev(fft32, x, win_len, hop, frames, max_mode=2, max_in=mx, **kw)
            assert given.tobytes() == one.tobytes() and bits_equal(mx2, mx)
            if depth == 8:
                for max_mode in (0, 1):
                    three, _ = run_dev(fft32, x, win_len, hop, frames, max_mode=max_mode, **kw)
                    four, _ = run_dev(fft32, x, win_len, hop, frames, max_mode=max_mode, **dict(kw, channels=4))
                    assert bits_equal(four[..., :3], three) and (four[..., 3] == 255).all()
    want, want_max, _ = po.expected(oracle, x, win_len, hop, frames, max_mode=0, mode=0, level=-100.0, cmap=so.FIRE, depth=8, channels=3, scale=0,
                                    layout=1)
    one, mx = run_dev(fft32, x, win_len, hop, frames, max_mode=0, mode=0, level=-100.0, cmap=so.FIRE, depth=8, channels=3, scale=0, layout=1)
    assert_pictures(one, want, "the chain's shape against the oracle")
    assert bits_equal(mx, want_max)


def test_special_values(fft32, oracle):
    """frontend_oracle.signal's zeros, subnormals, inf and NaN; a given maximum of 0, a negative value, NaN and a subnormal; level NaN."""
    rows, win_len, hop, frames = 4, 128, 32, 40
    x = fo.signal(seeded(68000), rows, frames * hop - 3)
    max_in = np.array([0.0, -2.0, np.nan, 1e-40], F)
    i = 0
    for max_mode in (0, 1, 2):
        for level in (-80.0, float("nan")):
            for mode in (0, 1):
                kw, host = options(i)
                i += 1
                kw.update(max_mode=max_mode, mode=mode, level=level)
                if max_mode == 1:
                    kw["scale"] = 0
                check(fft32, oracle, x, win_len, hop, frames, kw, host, "special values", max_in=max_in)


def _raw(f, sig, rows, length, stride, win, win_len, hop, frames, max_mode, max_in, max_out, out, mode=0, level=-80.0, cmap=0, depth=8, channels=3,
         scale=0, layout=1, table=None):
    vp = lambda p: None if not p else C.c_void_p(int(p))
    return f._lib.kofft_hip_dev_stft_picture_f32(f._ctx, vp(sig), rows, length, stride, vp(win), win_len, hop, frames, max_mode, vp(max_in),
                                                 vp(max_out), mode, level, cmap, depth, channels, scale, layout, table, vp(out))


@pytest.mark.parametrize("win_len,hop", [(128, 32), (1024, 256), (96, 40)])
def test_device_form_with_a_gap_between_the_rows(fft32, oracle, win_len, hop):
    """The signal 4 bytes past a 16-byte boundary, row_stride > len with NaN in the gaps (a frame at the end of a row reads +0, never the
    gap or the head of the next row), the pictures at an odd address and pre-filled."""
    import torch

    rows, frames, bins = 3, 19, win_len // 2
    length, stride = frames * hop - 5, frames * hop + 11
    x = fo.signal(seeded(69000 + win_len), rows, length)
    padded = np.full((rows, stride), np.nan, F)
    padded[:, :length] = x
    d = torch.full((rows * stride + 8,), float("nan"), device="cuda")
    d[1:1 + rows * stride] = torch.from_numpy(padded.reshape(-1)).cuda()
    for i in range(3):
        kw, _ = options(i + win_len)
        kw["scale"] = 0
        want, want_max, _ = po.expected(oracle, x, win_len, hop, frames, max_in=np.ones(rows, F), **kw)
        px = kw["channels"] * kw["depth"] // 8
        nbytes = rows * frames * bins * px
        out = torch.full((nbytes + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        mx = torch.full((rows,), float("nan"), device="cuda")
        ones = torch.ones(rows, device="cuda")
        torch.cuda.synchronize()
        off = 1 + i
        assert _raw(fft32, d.data_ptr() + 4, rows, length, stride, 0, win_len, hop, frames, kw["max_mode"], ones.data_ptr(), mx.data_ptr(),
                    out.data_ptr() + off, kw["mode"], kw["level"], kw["cmap"], kw["depth"], kw["channels"], 0, kw["layout"]) == 0
        fft32.synchronize()
        raw = out.cpu().numpy()
        assert (raw[:off] == 0xA5).all() and (raw[off + nbytes:] == 0xA5).all()
        got = raw[off:off + nbytes].copy().view(want.dtype).reshape(want.shape)
        assert_pictures(got, want, f"gap between rows, win_len {win_len}, {kw}")
        assert bits_equal(mx.cpu().numpy(), want_max)


def test_refusals_then_one_valid_call(fft32, oracle):
    import torch

    rows, length, win_len, hop, frames = 2, 640, 128, 64, 10
    x = fo.signal(seeded(70000), rows, length, special=False)
    d = torch.from_numpy(x).cuda()
    w = torch.from_numpy(np.hamming(win_len).astype(F)).cuda()
    mx = torch.full((rows,), 5.0, device="cuda")
    out = torch.full((rows * frames * 64 * 3,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sig, end = d.data_ptr(), d.data_ptr() + 4 * rows * length
    for o in (sig, sig + 400, end - 1):                      # the output inside the signal
        assert _raw(fft32, sig, rows, length, length, 0, win_len, hop, frames, 0, 0, 0, o) == 6
    assert _raw(fft32, sig, rows, length, length, w.data_ptr(), win_len, hop, frames, 1, 0, 0, w.data_ptr() + 4 * 127) == 6
    assert _raw(fft32, sig, rows, length, length, 0, win_len, hop, frames, 2, mx.data_ptr(), 0, mx.data_ptr() + 7) == 6
    assert _raw(fft32, sig, rows, length, length, 0, win_len, hop, frames, 0, 0, mx.data_ptr(), mx.data_ptr() - 100) == 6
    assert _raw(fft32, sig, rows, length, length, 0, win_len, hop, frames, 1, 0, 0, out.data_ptr(), scale=1,
                table=so.log_bin_map(64).ctypes.data_as(C.c_void_p)) == 6
    assert _raw(fft32, sig, rows, length, length, 0, win_len, hop, frames, 0, 0, 0, out.data_ptr(), channels=4, depth=16) == 6
    assert _raw(fft32, sig, rows, length, length, 0, win_len, hop, frames, 2, 0, 0, out.data_ptr()) == -3
    assert _raw(fft32, 0, 0, length, length, 0, win_len, hop, frames, 0, 0, 0, 0) == 0                                    # rows == 0
    # no bins: only max_out is written
    for max_mode, want in ((0, 0.0), (1, 1e-12), (2, 5.0)):
        m2 = torch.full((rows,), float("nan"), device="cuda")
        assert _raw(fft32, sig, rows, 6, 6, 0, 1, 2, 3, max_mode, mx.data_ptr(), m2.data_ptr(), out.data_ptr()) == 0
        fft32.synchronize()
        assert bits_equal(m2.cpu().numpy(), np.full(rows, want, F))
    fft32.synchronize()
    assert (out.cpu().numpy() == 0xA5).all() and bits_equal(d.cpu().numpy(), x) and (mx.cpu().numpy() == 5.0).all(), "the refused calls touched nothing"
    kw = dict(max_mode=0, mode=0, level=-80.0, cmap=so.FIRE, depth=8, channels=3, scale=0, layout=1)
    assert _raw(fft32, sig, rows, length, length, w.data_ptr(), win_len, hop, frames, 0, 0, mx.data_ptr(), out.data_ptr()) == 0
    fft32.synchronize()
    want, want_max, _ = po.expected(oracle, x, win_len, hop, frames, np.hamming(win_len).astype(F), **kw)
    assert_pictures(out.cpu().numpy().reshape(want.shape), want, "one valid call after the refusals")
    assert bits_equal(mx.cpu().numpy(), want_max)


def test_context_lifecycle_streams_and_the_python_module(oracle):
    """A second context, kofft_hip_release_scratch between calls, the device form from another stream, and kofft_amd.spectrogram.from_audio
    on numpy and on torch inputs."""
    import torch

    import kofft_amd
    from kofft_amd import spectrogram

    rows, win_len, hop, frames = 2, 256, 100, 11
    x = fo.signal(seeded(71000), rows, frames * hop - 9)
    c1, c2 = kofft_amd.HipFftImpl(F), kofft_amd.HipFftImpl(F)
    try:
        for i in range(4):
            kw, host = options(i)
            check(c1, oracle, x, win_len, hop, frames, kw, host, f"c1 call {i}")
            c1.release_scratch()
            check(c2, oracle, x, win_len, hop, frames, kw, not host, f"c2 call {i}")
        s = torch.cuda.Stream()
        c1.set_stream(s.cuda_stream)
        kw, _ = options(1)
        check(c1, oracle, x, win_len, hop, frames, kw, False, "another stream")
        c1.set_stream(0)
        for max_mode, name in ((0, "row"), (1, "running")):
            kw = dict(max_mode=max_mode, mode=0, level=-120.0, cmap=so.FIRE, depth=8, channels=3, scale=0, layout=1)
            want, want_max, _ = po.expected(oracle, x, win_len, hop, frames, **kw)
            got, mx = spectrogram.from_audio(x, win_len, hop, max_mode=name, fft=c1, return_max=True)
            assert_pictures(got, want, "from_audio, numpy")
            assert bits_equal(mx, want_max)
            one = spectrogram.from_audio(x[1], win_len, hop, max_mode=name, fft=c1)
            assert_pictures(one[None], want[1:2], "from_audio, one signal")
            t, tm = spectrogram.from_audio(torch.from_numpy(x).cuda(), win_len, hop, max_mode=name, fft=c1, return_max=True)
            c1.synchronize()
            assert_pictures(t.cpu().numpy(), want, "from_audio, torch")
            assert bits_equal(tm.cpu().numpy(), want_max)
        g = spectrogram.from_audio(x, win_len, hop, max_mode="given", max_mag=want_max, channels=4, layout="frames", cmap="rainbow", level=-80.0, fft=c2)
        want, _, _ = po.expected(oracle, x, win_len, hop, frames, max_mode=2, max_in=want_max, mode=0, level=-80.0, cmap=so.RAINBOW, depth=8,
                                 channels=4, scale=0, layout=0)
        assert_pictures(g, want, "from_audio, given")
    finally:
        c1.close()
        c2.close()
