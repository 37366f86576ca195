"""Every chunk loop of the host routes across its seams.  A route that works through a scratch buffer takes a large batch in pieces of at
most kofft_hip_ctx::scratch_chunk_bytes of it (scratch_chunk_rows, kofft_amd/csrc/host_layout.h) and rebases its input, scratch and output
pointers -- and sometimes a flat transform index -- for every piece.  At the default size (512 MiB) a seam needs a call of half a
gigabyte; KOFFT_HIP_SCRATCH_CHUNK_MB (read when a context is created) brings it down to a megabyte, so every case here makes its own
context, moves a few megabytes and crosses two full pieces and a ragged one (batch = 2 * chunk + r), often also chunk + 1 (a one-row
last piece) and a row larger than the cap (chunk == 1).  Every row is compared with the oracle, bit for bit.

`pieces()` restates the helper; each case asserts the split it means to cross, so a shape that stops crossing a seam fails here
instead of passing in one piece."""
import ctypes as C

import numpy as np
import pytest

from cepstrum_oracle import cepstrum_ref
from conftest import bits_equal, rand_c, seeded
from dct_oracle import dct2_ref
from onesided_ref import bins, complete
from rowcheck import assert_rows_equal
from split_oracle import split_ref

pytestmark = pytest.mark.gpu

KNOB = "KOFFT_HIP_SCRATCH_CHUNK_MB"
F32, F64 = np.float32, np.float64


def pieces(cap_mb, row_bytes, count):
    """The rows of every pass of a chunk loop: scratch_chunk_rows(cap, row_bytes, count) rows at a time."""
    chunk = max(1, min(count, (cap_mb << 20) // row_bytes))
    return [min(chunk, count - b0) for b0 in range(0, count, chunk)]


def chunk_kinds(t0, nt, frames):
    """The frames of the three kinds of rectangle that frame_cut (kofft_amd/csrc/frame_cut.h) makes of the chunk [t0, t0 + nt) of the
    flat index t = row * frames + frame: (the tail of a row the chunk does not begin, whole rows, the head of a row it does not end).
    A chunk inside one row counts as a tail (it begins inside the row) or a head (it begins the row)."""
    end, first = t0 + nt, -(-t0 // frames) * frames  # `first`: the first row start at or after t0
    if first >= end:
        return (nt, 0, 0) if t0 % frames else (0, 0, nt)
    whole = (end - first) // frames * frames
    return first - t0, whole, end - first - whole


def three_kind_chunks(cap_mb, frame_bytes, rows, frames):
    """The chunks (t0, nt) of scratch_chunk_rows(cap, frame_bytes, rows * frames) frames that hold all three kinds of rectangle, the
    whole rows being at least one.  A seam test of a framed family asserts that its geometry has one: a later change of a scratch
    layout then fails that precondition instead of quietly leaving the seam untested."""
    out, t0 = [], 0
    for nt in pieces(cap_mb, frame_bytes, rows * frames):
        if all(chunk_kinds(t0, nt, frames)):
            out.append((t0, nt))
        t0 += nt
    return out


def make(monkeypatch, dtype=F32, mb=1, **env):
    """A context created with the scratch cap at `mb` MiB (and further switches, e.g. BLUESTEIN_FUSED="0")."""
    import kofft_amd

    monkeypatch.setenv(KNOB, str(mb))
    for k, v in env.items():
        monkeypatch.setenv("KOFFT_HIP_" + k, v)
    return kofft_amd.HipFftImpl(dtype)


def _cdt(dt):
    return np.complex64 if dt == F32 else np.complex128


def _dev(a):
    """A device copy, complete before the context's own (non-blocking) stream may touch it."""
    import torch

    d = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return d


# ---- composed rfft / irfft (real_impl.hip.h: rfft_composed_dev, irfft_composed_dev) ---------------------------------------------------
def run_real(f, oracle, n, batch, windowed, seed, irfft=True):
    """rfft_batch of seeded rows (with a row window: the unfused window product puts z in front of y in the scratch; from m = 2^15 the
    window rides on the factor path's first load) and irfft_batch of the spectrum: every row against the oracle."""
    rng = seeded(seed)
    rows = rng.uniform(-1, 1, (batch, n)).astype(f.dtype)
    win = rng.uniform(0.1, 1, n).astype(f.dtype) if windowed else None
    what = f"{f.dtype.name} n={n} batch={batch}{' windowed' if windowed else ''}"
    spec = f.rfft_batch(rows, win)
    assert_rows_equal(spec, oracle.rfft_mt(rows, win), "rfft " + what)
    if irfft:
        assert_rows_equal(f.irfft_batch(spec, n), oracle.irfft_mt(spec, n), "irfft " + what)


REAL_CASES = [
    # (dtype, n, batch, the pieces at 1 MiB)                       m = n / 2
    (F32, 1000, 561, [262, 262, 37]),   # m = 500: the flat post / pre kernels
    (F32, 1000, 263, [262, 1]),
    (F64, 1000, 299, [131, 131, 37]),
    (F64, 1000, 132, [131, 1]),
    (F32, 1200, 441, [218, 218, 5]),    # m = 600: the grid.y kernels
    (F64, 1200, 223, [109, 109, 5]),
    (F32, 1 << 17, 5, [2, 2, 1]),       # m = 2^16: the factor path inside, the window on its first load
    (F32, 1 << 19, 3, [1, 1, 1]),       # one row (2 MiB) exceeds the cap
    (F64, 1 << 19, 3, [1, 1, 1]),
]


@pytest.mark.parametrize("dt,n,batch,want", REAL_CASES, ids=[f"{np.dtype(d).name}-{n}x{b}" for d, n, b, _ in REAL_CASES])
def test_composed_rfft_and_irfft_across_chunk_seams(oracle, monkeypatch, dt, n, batch, want):
    assert pieces(1, n * np.dtype(dt).itemsize, batch) == want
    f = make(monkeypatch, dt)
    try:
        for windowed in (False, True):
            run_real(f, oracle, n, batch, windowed, 71000 + n % 997 + batch)
    finally:
        f.close()


@pytest.mark.parametrize("dt,n", [(F32, 65536), (F64, 32768)], ids=["f32-65536", "f64-32768"])
@pytest.mark.parametrize("epi", ["1", "0"], ids=["one-pass", "two-passes"])
def test_real_transforms_with_two_routes_in_one_call(oracle, monkeypatch, dt, n, epi):
    """m = 2^15 (f32) / 2^14 (f64) with the cap at 160 MiB: 710 rows are one piece of 640 rows -- at least two per CU, the register-file
    route (RfftRowIO; with KOFFT_HIP_RFFT_REGFILE_EPI=0 RowWindowIO for the windowed call and the plain register-file transform, each
    followed by the post-pass kernel; IrfftRowIO) -- and a piece of 70 rows on the route below it (the factor path and the separate
    pre- / post-pass kernels), both writing into the same output.  (The inverse does not read the epilogue switch: once.)"""
    import torch

    batch = 710
    assert pieces(160, n * np.dtype(dt).itemsize, batch) == [640, 70]
    assert 70 < 2 * torch.cuda.get_device_properties(0).multi_processor_count <= 640
    f = make(monkeypatch, dt, mb=160, RFFT_REGFILE_EPI=epi)
    try:
        run_real(f, oracle, n, batch, False, 72000 + n, irfft=epi == "1")
        run_real(f, oracle, n, batch, True, 72001 + n, irfft=False)
    finally:
        f.close()


# ---- DCT-II composed (dct_impl.hip.h: dct2_composed_dev) ------------------------------------------------------------------------------
def run_dct(f, n, batch, seed, misalign=False):
    """dct2_batch (or, misalign: dct2_dev on an input that is 4 mod 8, which takes the composed route at every length) against the
    oracle, every row."""
    import torch

    x = seeded(seed).uniform(-1, 1, (batch, n)).astype(F32)
    if not misalign:
        got = f.dct2_batch(x)
    else:
        d = torch.empty(batch * n + 3, dtype=torch.float32, device="cuda")
        off = 1 if d.data_ptr() % 8 == 0 else 2
        src = d[off:off + batch * n]
        assert src.data_ptr() % 8 == 4
        src.copy_(torch.from_numpy(x.reshape(-1)))
        d_out = torch.full((batch, n), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # (torch's copies and fills run on its stream, the call on the context's own)
        f.dct2_dev(src.data_ptr(), d_out.data_ptr(), n, batch)
        f.synchronize()
        got = d_out.cpu().numpy()
    assert_rows_equal(got, dct2_ref(x), f"dct2 n={n} batch={batch}{' (input 4 mod 8)' if misalign else ''}")


DCT_CASES = [
    # (n, batch, the pieces at 1 MiB: rows of 2n floats, misaligned input)
    (100, 2743, [1310, 1310, 123], False),  # the flat mirror / post kernels, Bluestein (m = 256) inside
    (100, 1311, [1310, 1], False),
    (1000, 299, [131, 131, 37], False),     # Bluestein inside
    (1001, 297, [130, 130, 37], False),     # odd n: no 8-byte loads
    (8192, 37, [16, 16, 5], False),         # a power of two beyond the fused sizes
    (8192, 17, [16, 1], False),
    (1024, 265, [128, 128, 9], True),       # a fused length on the composed route
    (1 << 18, 3, [1, 1, 1], False),         # one mirrored row (2 MiB) exceeds the cap; the factor path inside
]


@pytest.mark.parametrize("n,batch,want,misalign", DCT_CASES, ids=[f"{n}x{b}" for n, b, _, _ in DCT_CASES])
def test_composed_dct2_across_chunk_seams(oracle, monkeypatch, n, batch, want, misalign):
    assert pieces(1, 2 * n * 4, batch) == want
    f = make(monkeypatch)
    try:
        run_dct(f, n, batch, 73000 + n % 991 + batch, misalign)
    finally:
        f.close()


def test_composed_dct2_with_the_bluestein_loop_inside_its_own(oracle, monkeypatch):
    """n = 20000, 13 rows: DCT pieces of 6, 6 and 1 rows, and inside each the n-point transform is Bluestein's at m = 65536 (512 KiB
    per transform), which runs its own loop over blue_tmp in pieces of 2."""
    assert pieces(1, 2 * 20000 * 4, 13) == [6, 6, 1] and pieces(1, 65536 * 8, 6) == [2, 2, 2]
    f = make(monkeypatch)
    try:
        run_dct(f, 20000, 13, 73500)
    finally:
        f.close()


# ---- planar fft_split / ifft_split composed (planar_impl.hip.h: planar_composed_dev) ----------------------------------------------------
def run_planar(f, n, batch, seed, dev_forms=True):
    """fft_split_batch forward and inverse (host form, in place) and the in-place and out-of-place device forms: every row of both
    planes against the oracle; the out-of-place form leaves its inputs alone."""
    rng = seeded(seed)
    re, im = rng.uniform(-1, 1, (batch, n)).astype(f.dtype), rng.uniform(-1, 1, (batch, n)).astype(f.dtype)
    for inverse in (False, True):
        what = f"split {f.dtype.name} n={n} batch={batch} inverse={inverse}"
        want = split_ref(re, im, inverse)
        a, b = re.copy(), im.copy()
        f.fft_split_batch(a, b, inverse)
        assert_rows_equal(a, want[0], what + " re")
        assert_rows_equal(b, want[1], what + " im")
        if not dev_forms:
            continue
        d_re, d_im = _dev(re), _dev(im)
        o_re, o_im = _dev(np.full_like(re, np.nan)), _dev(np.full_like(im, np.nan))
        f.fft_split_dev(d_re, d_im, o_re, o_im, inverse=inverse)
        f.synchronize()
        assert_rows_equal(o_re.cpu().numpy(), want[0], what + " re, out of place")
        assert_rows_equal(o_im.cpu().numpy(), want[1], what + " im, out of place")
        assert bits_equal(d_re.cpu().numpy(), re) and bits_equal(d_im.cpu().numpy(), im), what + ": an input plane changed"
        f.fft_split_dev(d_re, d_im, inverse=inverse)
        f.synchronize()
        assert_rows_equal(d_re.cpu().numpy(), want[0], what + " re, in place")
        assert_rows_equal(d_im.cpu().numpy(), want[1], what + " im, in place")


PLANAR_CASES = [
    # (dtype, n, batch, the pieces at 1 MiB, fused route off)
    (F32, 1000, 299, [131, 131, 37], False),
    (F32, 1000, 132, [131, 1], False),
    (F64, 1000, 167, [65, 65, 37], False),
    (F32, 256, 1030, [512, 512, 6], True),
    (F64, 256, 518, [256, 256, 6], True),
    (F32, 1 << 18, 3, [1, 1, 1], False),  # one row (2 MiB) exceeds the cap
]


@pytest.mark.parametrize("dt,n,batch,want,unfused", PLANAR_CASES, ids=[f"{np.dtype(d).name}-{n}x{b}" for d, n, b, _, _ in PLANAR_CASES])
def test_composed_planar_transforms_across_chunk_seams(oracle, monkeypatch, dt, n, batch, want, unfused):
    assert pieces(1, n * 2 * np.dtype(dt).itemsize, batch) == want
    f = make(monkeypatch, dt)
    try:
        if unfused:
            f.set_split_fused(False)
        run_planar(f, n, batch, 74000 + n % 983 + batch)
    finally:
        f.close()


# ---- cepstrum composed (cepstrum_impl.hip.h: cepstrum_composed_dev) -----------------------------------------------------------------
CEPSTRUM_CASES = [
    # (n, batch, the pieces at 1 MiB, fused route off).  real_cepstrum takes powers of two only (cepstrum.rs:16), so n = 1000 never
    # reaches the loop: the composed lengths nearest to it are 8192 (the first beyond the fused sizes) and 16 (the last below them).
    (8192, 37, [16, 16, 5], False),
    (8192, 17, [16, 1], False),
    (16, 16500, [8192, 8192, 116], False),
    (256, 1030, [512, 512, 6], True),
    (1 << 18, 3, [1, 1, 1], False),  # one row (2 MiB) exceeds the cap
]


@pytest.mark.parametrize("n,batch,want,unfused", CEPSTRUM_CASES, ids=[f"{n}x{b}" for n, b, _, _ in CEPSTRUM_CASES])
def test_composed_cepstrum_across_chunk_seams(oracle, monkeypatch, n, batch, want, unfused):
    assert pieces(1, n * 8, batch) == want
    f = make(monkeypatch)
    try:
        if unfused:
            f.set_cepstrum_fused(False)
        x = seeded(75000 + n % 977 + batch).uniform(-1, 1, (batch, n)).astype(F32)
        assert_rows_equal(f.cepstrum_batch(x), cepstrum_ref(x), f"cepstrum n={n} batch={batch}")
    finally:
        f.close()


# ---- Bluestein's loop over blue_tmp (complex_impl.hip.h: fft_bluestein_dev) ---------------------------------------------------------
def run_complex(f, oracle, n, batch, seed):
    """fft_batch and ifft_batch of its result, every row against the oracle."""
    x = rand_c(seeded(seed), (batch, n), _cdt(f.dtype))
    y = x.copy()
    f.fft_batch(y)
    want = oracle.fft_mt(x)
    what = f"{y.dtype.name} n={n} batch={batch}"
    assert_rows_equal(y, want, what + ": forward")
    f.fft_batch(y, inverse=True)
    assert_rows_equal(y, oracle.fft_mt(want, inverse=True), what + ": inverse")


BLUESTEIN_CASES = [
    # (dtype, n, m, batch, the pieces at 1 MiB, KOFFT_HIP_BLUESTEIN_FUSED)
    (F32, 5000, 16384, 19, [8, 8, 3], "1"),   # the fused first / second kernels through the scratch
    (F32, 5000, 16384, 9, [8, 1], "1"),
    (F64, 2500, 8192, 19, [8, 8, 3], "1"),    # ... in f64 (m = 2^13, its largest)
    (F32, 20000, 65536, 5, [2, 2, 1], "1"),   # m beyond one workgroup: the pointwise steps on the factor kernels
    (F64, 5000, 16384, 11, [4, 4, 3], "1"),
    (F32, 1000, 2048, 133, [64, 64, 5], "0"),  # the three pointwise kernels around two plain transforms
    (F64, 1000, 2048, 69, [32, 32, 5], "0"),
    (F64, 40000, 131072, 3, [1, 1, 1], "1"),  # one padded transform (2 MiB) exceeds the cap
]


@pytest.mark.parametrize("dt,n,m,batch,want,fused", BLUESTEIN_CASES,
                         ids=[f"{np.dtype(d).name}-{n}x{b}-fused{fu}" for d, n, _, b, _, fu in BLUESTEIN_CASES])
def test_bluestein_loop_across_chunk_seams(oracle, monkeypatch, dt, n, m, batch, want, fused):
    """Lengths whose padded length m no one-launch Bluestein kernel serves at these batches (c32: m = 16384 and beyond; c64: 8192 and
    beyond; every m with the fused steps switched off)."""
    assert m >= 2 * n - 1 > m // 2 and pieces(1, m * 2 * np.dtype(dt).itemsize, batch) == want
    f = make(monkeypatch, dt, BLUESTEIN_FUSED=fused)
    try:
        run_complex(f, oracle, n, batch, 76000 + n % 971 + batch)
    finally:
        f.close()


# ---- the radix-4 arm (complex_impl.hip.h: fft_radix4_dev) ---------------------------------------------------------------------------
def _plan_ifft(x, forward):
    """FftPlan::ifft (fft.rs:2040-2055) around `forward`: conj, forward, conj * 1 / (n as f32), element by element."""
    real = F32 if x.dtype == np.complex64 else F64
    y = forward(np.conj(x))
    scale = real(1) / real(np.float32(x.shape[-1]))
    out = np.empty_like(y)
    out.real = y.real * scale
    out.imag = (-y.imag) * scale
    return out


RADIX4_CASES = [
    (F32, 256, 1030, [512, 512, 6]),
    (F32, 256, 513, [512, 1]),
    (F64, 256, 518, [256, 256, 6]),
    (F32, 1024, 263, [128, 128, 7]),
    (F64, 1024, 135, [64, 64, 7]),
    (F32, 1 << 18, 3, [1, 1, 1]),  # 4^9 points: one transform (2 MiB) exceeds the cap
]


@pytest.mark.parametrize("dt,n,batch,want", RADIX4_CASES, ids=[f"{np.dtype(d).name}-{n}x{b}" for d, n, b, _ in RADIX4_CASES])
def test_radix4_arm_across_chunk_seams(oracle, monkeypatch, dt, n, batch, want):
    """fft_radix4_batch and the plan's inverse around it, in a context with the compat default and in one with radix4_compat=False
    (the flag decides what fft_with_strategy calls, not what the arm computes: the same bytes from both)."""
    import kofft_amd

    assert pieces(1, n * 2 * np.dtype(dt).itemsize, batch) == want
    monkeypatch.setenv(KNOB, "1")
    x = rand_c(seeded(77000 + n % 967 + batch), (batch, n), _cdt(dt))
    want_fwd, want_inv = oracle.fft_radix4(x), _plan_ifft(x, oracle.fft_radix4)
    for compat in (None, False):
        f = kofft_amd.HipFftImpl(dt, radix4_compat=compat)
        try:
            assert f.radix4_compat is (compat is None)
            y = x.copy()
            f.fft_radix4_batch(y)
            assert_rows_equal(y, want_fwd, f"fft_radix4 {y.dtype.name} n={n} batch={batch} compat={compat}")
            y = x.copy()
            f._check(f._fn(f"ifft_radix4_{f._cplx}")(f._ctx, C.c_void_p(y.ctypes.data), n, batch))
            assert_rows_equal(y, want_inv, f"ifft_radix4 {y.dtype.name} n={n} batch={batch} compat={compat}")
        finally:
            f.close()


# ---- N-D (complex_impl.hip.h: fft_axis2_core; k_nd.hip: the transpose panels) -----------------------------------------------------------
def run_nd(f, oracle, depth, rows, cols, seed):
    """fftnd forward and inverse of a seeded volume against the oracle's transform along each axis (z, y, x: ndfft.rs:131-151)."""
    cdt = _cdt(f.dtype)
    x = rand_c(seeded(seed), (depth, rows, cols), cdt)

    def axis(a, ax, inverse):
        moved = np.ascontiguousarray(np.moveaxis(a, ax, -1))
        out = oracle.fft_mt(moved.reshape(-1, moved.shape[-1]), inverse=inverse).reshape(moved.shape)
        return np.ascontiguousarray(np.moveaxis(out, -1, ax))

    data = x.reshape(-1).copy()
    want = x
    for inverse in (False, True):
        for ax in (0, 1, 2):
            want = axis(want, ax, inverse)
        f.fftnd(data, depth, rows, cols, inverse=inverse)
        assert_rows_equal(data.reshape(depth * rows, cols), want.reshape(depth * rows, cols),
                          f"fftnd {depth}x{rows}x{cols} {np.dtype(cdt).name} inverse={inverse}")


@pytest.mark.parametrize("dt,shape,want", [(F32, (5, 4096, 128), [2, 2, 1]), (F64, (3, 4096, 128), [1, 1, 1])], ids=["c32", "c64"])
def test_nd_two_pass_axis_across_chunk_seams(oracle, monkeypatch, dt, shape, want):
    """The cap at 8 MiB.  The 4096-point y axis over 128 adjacent lines takes the two column-tile passes (fft_axis2_core) from 16 MiB
    of lines on: c32 five blocks of 4 MiB in pieces of 2, 2 and 1; c64 three blocks of 8 MiB -- the smallest volume with three pieces
    (two blocks are the 16 MiB the route starts at) -- one per piece, each filling the cap.  The z axis (5 or 3 points: Bluestein)
    goes through the transpose panels (16 MiB) in two panels, and Bluestein's own loop inside them."""
    depth, rows, cols = shape
    block = rows * cols * 2 * np.dtype(dt).itemsize
    assert depth * block >= 16 << 20 and pieces(8, block, depth) == want
    f = make(monkeypatch, dt, mb=8)
    try:
        run_nd(f, oracle, depth, rows, cols, 78000 + depth)
    finally:
        f.close()


ND_PANEL_CASES = [
    # (dtype, (depth, rows, cols), panel widths P of the y axis, outer blocks per group OG)  -- the cap is 2 * 1 MiB
    (F32, (3, 1000, 300), [256, 44], [1, 1, 1]),
    (F32, (5, 3000, 40), [32, 8], [2, 2, 1]),
    (F64, (3, 1000, 300), [128, 128, 44], [1, 1, 1]),
]


@pytest.mark.parametrize("dt,shape,panels,groups", ND_PANEL_CASES, ids=["c32-3x1000x300", "c32-5x3000x40", "c64-3x1000x300"])
def test_nd_transpose_panels_across_their_seams(oracle, monkeypatch, dt, shape, panels, groups):
    """The y axis (1000 or 3000 points: no strided kernel, so transposes at every size) in panels of P columns by OG outer blocks; the z
    axis (3 or 5 points over rows * cols adjacent lines) in several panels too; Bluestein's loop runs inside the panels."""
    depth, rows, cols = shape
    cap, col_bytes = 2 << 20, rows * 2 * np.dtype(dt).itemsize
    p = min(cap // col_bytes, cols)
    p = p & ~31 if p >= 32 else max(p, 1)
    og = max(1, min(cap // (p * col_bytes), depth))
    assert [min(p, cols - c) for c in range(0, cols, p)] == panels and [min(og, depth - o) for o in range(0, depth, og)] == groups
    f = make(monkeypatch, dt)
    try:
        run_nd(f, oracle, depth, rows, cols, 79000 + rows + cols)
    finally:
        f.close()


# ---- the composed STFT and the magnitudes of one signal (k_stft.hip: stft_composed_dev, stft_mag_dev) -------------------------------------
@pytest.mark.parametrize("win_len,hop,frames,want", [(1000, 300, 299, [131, 131, 37]), (1000, 300, 132, [131, 1]),
                                                     (12, 5, 21900, [10922, 10922, 56])], ids=["1000", "1000-one-frame-piece", "12"])
def test_composed_stft_of_one_signal_across_chunk_seams(oracle, monkeypatch, win_len, hop, frames, want):
    """Window lengths that are no power of two, hops that do not divide them, a signal that ends inside the last frames (they are
    zero-padded), and fewer frames than the persistent Bluestein kernel takes (1024 at m = 2048, 65536 at m = 32 on 256 CUs), so
    stft_into runs stft_composed_dev's loop; stft_magnitudes runs its own loop around single pieces of it, the maximum (the samples
    of the last piece's frames are three times larger) merged over all of them."""
    assert pieces(1, win_len * 8, frames) == want
    f = make(monkeypatch)
    try:
        rng = seeded(80000 + win_len + frames)
        length = (frames - 1) * hop + hop // 2
        assert -(-length // hop) == frames and length < (frames - 2) * hop + win_len
        sig = rng.uniform(-1, 1, length).astype(F32)
        sig[(frames - want[-1]) * hop:] *= np.float32(3)
        win = rng.uniform(0.1, 1, win_len).astype(F32)
        assert_rows_equal(f.stft_into(sig, win, hop, frames), oracle.stft(sig, win, hop, frames), f"stft win {win_len} hop {hop}")
        mags, mx = f.stft_magnitudes(sig, win_len, hop)
        want_m, want_x = oracle.stft_magnitudes(sig, win_len, hop)
        assert_rows_equal(mags, want_m, f"magnitudes win {win_len} hop {hop}")
        assert np.float32(mx).tobytes() == np.float32(want_x).tobytes(), f"maximum {mx} want {want_x}"
        if len(want) == 3:
            assert np.argmax(want_m.max(axis=1)) >= want[0] + want[1] - 3, "the maximum does not come from the last pieces"
    finally:
        f.close()


# ---- STFT over rows, composed (k_stft_rows.hip, k_stft_onesided.hip: the loops over the flat transform index) ----------------------------
def test_composed_stft_rows_across_chunk_seams_inside_rows(oracle, monkeypatch):
    """win_len = 1000, 7 rows of 50 frames: 350 transforms in pieces of 131, 131 and 88, the seams inside rows 2 and 5.  stft_rows,
    stft_onesided and stft_magnitudes_rows, host forms and device forms with row_stride > len (NaN in the gaps).  Every row's samples
    from frame 40 on are five times larger, so the maxima of rows 2 and 5 come from the piece after the one that holds their first
    frames; the maxima are compared bit for bit."""
    from test_gpu_stft_onesided import _onesided_dev
    from test_gpu_stft_rows import _mag_ref, _mag_rows_dev, _stft_ref, _stft_rows_dev

    win_len, hop, rows, frames = 1000, 300, 7, 50
    assert pieces(1, win_len * 8, rows * frames) == [131, 131, 88] and 131 // frames == 2 and 262 // frames == 5
    # the second piece holds all three kinds of rectangle: the tail of row 2, rows 3 and 4, the head of row 5 (framed_produce's cells
    # "full frames, composed" and "kept bins, composed")
    assert three_kind_chunks(1, win_len * 8, rows, frames) == [(131, 131)] and chunk_kinds(131, 131, frames) == (19, 100, 12)
    f = make(monkeypatch)
    try:
        rng = seeded(81000)
        length = (frames - 1) * hop + hop // 2
        x = (rng.uniform(-1, 1, (rows, length)) * (1.0 + np.arange(rows))[:, None]).astype(F32)
        x[:, 40 * hop:] *= np.float32(5)
        win = rng.uniform(0.1, 1, win_len).astype(F32)
        want = _stft_ref(oracle, x, win, hop, frames)
        k = bins(win_len)
        flat = lambda a: a.reshape(rows * frames, -1)
        assert_rows_equal(flat(f.stft_rows(x, win, hop)), flat(want), "stft_rows, host form")
        assert_rows_equal(flat(_stft_rows_dev(f, x, length + 7, win, hop, frames)), flat(want), "stft_rows, device form, stride len + 7")
        assert_rows_equal(flat(f.stft_onesided(x, win, hop)), flat(want[:, :, :k]), "stft_onesided, host form")
        assert_rows_equal(flat(_onesided_dev(f, x, length + 7, win, hop, frames)), flat(want[:, :, :k]), "stft_onesided, device form")
        want_m, want_x = _mag_ref(oracle, x, win_len, hop)
        for r, seam in ((2, 131), (5, 262)):
            first_piece = want_m[r, :seam - r * frames].max()
            assert want_x[r] == want_m[r, seam - r * frames:].max() > first_piece, f"row {r}: the maximum lies before the seam"
        for mags, mx in (f.stft_magnitudes_rows(x, win_len, hop), _mag_rows_dev(f, x, length + 7, win_len, hop, frames)):
            assert_rows_equal(flat(mags), flat(want_m), "stft_magnitudes_rows")
            assert bits_equal(mx, want_x), f"maxima {mx} want {want_x}"
    finally:
        f.close()


# ---- ISTFT over rows with the caller's frames kept (k_stft_rows.hip: istft_rows_dev's walk over whole rows) -------------------------------
def inverse_parallel_ref(oracle, spec, win, hop, pre):
    """stft::inverse_parallel (stft.rs:289-343) per row, from the oracle's inverse transforms: every sample accumulates
    frame[f][i].re * window[i] onto what the output held, frames in increasing order, one float32 rounding per operation; the sum
    is divided by the window-square sum where that exceeds 1e-8, and is 0 elsewhere."""
    rows, nfr, n = spec.shape
    out_len = pre.shape[1]
    time = oracle.fft_mt(spec.reshape(rows * nfr, n), inverse=True).reshape(rows, nfr, n).real
    acc, norm = pre.astype(F32).copy(), np.zeros(out_len, F32)
    for fi in range(nfr):
        lo = fi * hop
        hi = min(lo + n, out_len)
        if hi <= lo:
            break
        acc[:, lo:hi] = acc[:, lo:hi] + time[:, fi, :hi - lo] * win[:hi - lo]
        norm[lo:hi] = norm[lo:hi] + win[:hi - lo] * win[:hi - lo]
    ok = norm > np.float32(1e-8)
    out = np.zeros_like(acc)
    out[:, ok] = acc[:, ok] / norm[ok]
    return out


@pytest.mark.parametrize("win_len,hop,frames,rows,want", [(64, 24, 100, 47, [20, 20, 7]), (64, 24, 100, 21, [20, 1]),
                                                          (1024, 200, 200, 3, [1, 1, 1])], ids=["64x100x47", "64x100x21", "1024x200x3"])
def test_istft_rows_with_kept_frames_across_chunk_seams(oracle, monkeypatch, win_len, hop, frames, rows, want):
    """inverse_parallel over rows on device pointers and istft_onesided (host and device forms) walk whole rows through rows_tmp: 20
    rows of 100 x 64 frames per pass, or one row where a row alone (200 x 1024: 1.6 MB) exceeds the cap.  The output held non-zero
    values beforehand (the overlap-add accumulates), a few samples past the frames' cover included; the caller's frames are unchanged."""
    assert pieces(1, frames * win_len * 8, rows) == want
    f = make(monkeypatch)
    try:
        rng = seeded(82000 + win_len + rows)
        out_len = (frames - 1) * hop + win_len + 5
        win = rng.uniform(0.1, 1, win_len).astype(F32)
        pre = rng.uniform(-1, 1, (rows, out_len)).astype(F32)
        half = rand_c(rng, (rows, frames, bins(win_len)))
        full = complete(half, win_len)
        want_out = inverse_parallel_ref(oracle, full, win, hop, pre)
        assert not want_out[:, -5:].any() and want_out[:, :-5].all()
        d_win = _dev(win)
        # the full frames, kept
        d_fr, d_out = _dev(full.view(F32)), _dev(pre)
        f.istft_rows_dev(d_fr.data_ptr(), rows, frames, d_win.data_ptr(), win_len, hop, d_out.data_ptr(), out_len, parallel=True)
        f.synchronize()
        assert_rows_equal(d_out.cpu().numpy(), want_out, "istft_rows_dev, parallel")
        assert bits_equal(d_fr.cpu().numpy(), full.view(F32)), "istft_rows_dev, parallel: the caller's frames changed"
        # the one-sided frames: device form, then host form
        d_half, d_out = _dev(half.view(F32)), _dev(pre)
        f.istft_onesided_dev(d_half.data_ptr(), rows, frames, d_win.data_ptr(), win_len, hop, d_out.data_ptr(), out_len)
        f.synchronize()
        assert_rows_equal(d_out.cpu().numpy(), want_out, "istft_onesided_dev")
        assert bits_equal(d_half.cpu().numpy(), half.view(F32)), "istft_onesided_dev: the caller's frames changed"
        out, keep = pre.copy(), half.copy()
        f.istft_onesided(keep, win, hop, out)
        assert_rows_equal(out, want_out, "istft_onesided, host form")
        assert bits_equal(keep, half)
    finally:
        f.close()


# ---- one context, several families -----------------------------------------------------------------------------------------------------
def test_scratch_is_regrown_and_repointed_between_families(oracle, monkeypatch):
    """One context with the cap at 1 MiB: a DCT, a planar transform and a windowed rfft back to back grow real_tmp (and lay it out
    differently: the rfft puts the windowed rows in front of the spectrum), each in three pieces; then release_scratch and the first
    case again from nothing."""
    f = make(monkeypatch)
    try:
        run_dct(f, 1000, 299, 83001)
        run_planar(f, 1000, 299, 83002, dev_forms=False)
        run_real(f, oracle, 1000, 561, True, 83003)
        f.release_scratch()
        run_dct(f, 1000, 299, 83001)
    finally:
        f.close()


def knob_case(oracle):
    """tests/test_gpu_knobs.py's row for KOFFT_HIP_SCRATCH_CHUNK_MB=1 (set by the caller): contexts created now cut at 1 MiB."""
    import kofft_amd

    for dt, n, batch in ((F32, 1000, 561), (F64, 1200, 223)):
        f = kofft_amd.HipFftImpl(dt)
        try:
            run_real(f, oracle, n, batch, True, 84000 + n)
            run_complex(f, oracle, 5000 if dt == F32 else 2500, 19, 84100 + n)
        finally:
            f.close()
