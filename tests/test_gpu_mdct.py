"""The fast DCT-IV, MDCT and IMDCT of DESIGN.md 5.32 on the device, bit for bit against tests/mdct_oracle.py.  N = 64 .. 8192 a power
of two runs dct4_fused_kernel<5 .. 12, IO> (one launch per DCT-IV; the MDCT's window and fold on its loads); every other N -- and every N
in a context with set_mdct_fused(False) -- runs dct4_pre_kernel -> fft_dev -> dct4_post_kernel through the context's scratch.  The IMDCT
adds imdct_ola_kernel.  Every call runs twice and its two results are compared; the default context and the composed one get the same
inputs and must give the same bytes."""
import numpy as np
import pytest

from conftest import bits_equal, seeded
import mdct_oracle as mo
from rowcheck import assert_rows_equal
from test_mdct_cpu import ROUND_TRIP, rel

pytestmark = pytest.mark.gpu
F = np.float32
XPB = {5: 32, 6: 16, 7: 16, 8: 16, 9: 4, 10: 4, 11: 2, 12: 1}  # items per workgroup of the fused kernel, by log2 (N / 2)
FUSED_N = [64 << i for i in range(8)]
COMPOSED_N = [2, 32, 240, 960, 16384]


@pytest.fixture(scope="module")
def composed32():
    """A context with the fused route off (set_mdct_fused(False)): every transform through the composed route."""
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_mdct_fused(False)
    yield f
    f.close()


def _sine(n):
    from kofft_amd import mdct as km

    return km.sine_window(n)


def _twice(call, what):
    a, b = call(), call()
    assert bits_equal(a, b), what + ": two runs of the same call differ"
    return a


def _up(a, off=0, fill=0.0):
    import torch

    a = np.ascontiguousarray(a, F)
    d = torch.full((a.size + off,), fill, dtype=torch.float32, device="cuda")
    d[off:] = torch.from_numpy(a.reshape(-1)).cuda()
    return d


def _dct4_dev(f, u, off=0, in_place=False):
    import torch

    rows, n = u.shape
    res = []
    for _ in range(2):
        dx = _up(u, off)
        out = dx if in_place else torch.full((u.size + off,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # (the context's stream does not wait for torch's)
        f.dct4_fast_dev(dx.data_ptr() + 4 * off, out.data_ptr() + 4 * off, n, rows)
        f.synchronize()
        res.append(out[off:].cpu().numpy().reshape(rows, n))
    assert bits_equal(res[0], res[1]), "dct4_fast_dev: two runs of the same call differ"
    return res[0]


def _mdct_dev(f, x, w, lead, frames, stride=None, off=0):
    """x: [rows, nx]; stride > nx: the gaps between the rows (and behind the last) hold NaN."""
    import torch

    rows, nx = x.shape
    n = w.size // 2
    stride = nx if stride is None else stride
    padded = np.full((rows, stride), np.nan, F)
    padded[:, :nx] = x
    dx, dw = _up(padded, off, fill=float("nan")), _up(w, off)
    res = []
    for _ in range(2):
        out = torch.full((rows * frames * n,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # (the context's stream does not wait for torch's)
        f.mdct_dev(dx.data_ptr() + 4 * off, rows, nx, stride, dw.data_ptr() + 4 * off, n, lead, out.data_ptr(), frames)
        f.synchronize()
        res.append(out.cpu().numpy().reshape(rows, frames, n))
    assert bits_equal(res[0], res[1]), "mdct_dev: two runs of the same call differ"
    return res[0]


def _imdct_dev(f, X, w, scale, first, count):
    import torch

    rows, frames, n = X.shape
    dX, dw = _up(X), _up(w)
    res = []
    for _ in range(2):
        out = torch.full((rows * count,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # (the context's stream does not wait for torch's)
        f.imdct_dev(dX.data_ptr(), rows, frames, dw.data_ptr(), n, scale, out.data_ptr(), first, count)
        f.synchronize()
        res.append(out.cpu().numpy().reshape(rows, count))
    assert bits_equal(res[0], res[1]), "imdct_dev: two runs of the same call differ"
    return res[0]


def _both(fft32, composed32, run, want, what, nan_safe=False):
    got = run(fft32)
    assert_rows_equal(got.reshape(want.shape[0], -1), want.reshape(want.shape[0], -1), what + ": default route", nan_safe=nan_safe)
    got_c = run(composed32)
    assert_rows_equal(got_c.reshape(want.shape[0], -1), want.reshape(want.shape[0], -1), what + ": composed route", nan_safe=nan_safe)
    if not nan_safe:
        assert bits_equal(got, got_c), what + ": the two routes differ"


# ---- DCT-IV rows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", FUSED_N)
def test_dct4_fused_ladder(fft32, composed32, oracle, n):
    """Every fused instance with XPB + 1 and 2 XPB + 1 rows: more than one workgroup, the last one partly empty."""
    xpb = XPB[(n // 2).bit_length() - 1]
    for rows in (xpb + 1, 2 * xpb + 1):
        u = seeded(12000 + n + rows).uniform(-1, 1, (rows, n)).astype(F)
        want = mo.dct4_ref(u)
        _both(fft32, composed32, lambda f: _dct4_dev(f, u), want, f"dct4 N={n} rows={rows} dev")
        _both(fft32, composed32, lambda f: _twice(lambda: f.dct4_fast_batch(u), "dct4_fast_batch"), want, f"dct4 N={n} rows={rows} host")


@pytest.mark.parametrize("n", [2, 4, 8, 16, 32, 6, 240, 960, 16384, 1 << 17])
def test_dct4_composed_lengths(fft32, composed32, oracle, n):
    rows = 5 if n <= 960 else 2
    u = seeded(12100 + n).uniform(-1, 1, (rows, n)).astype(F)
    want = mo.dct4_ref(u)
    _both(fft32, composed32, lambda f: _dct4_dev(f, u), want, f"dct4 N={n} dev")
    _both(fft32, composed32, lambda f: _twice(lambda: f.dct4_fast_batch(u), "dct4_fast_batch"), want, f"dct4 N={n} host")


@pytest.mark.parametrize("n", [64, 1024, 8192, 240])
def test_dct4_in_place_and_unaligned(fft32, composed32, oracle, n):
    """d_out == d_in on both routes; buffers one float into their allocations (still 4-byte aligned); and, through the module, any
    leading shape."""
    from kofft_amd import mdct as km

    u = seeded(12200 + n).uniform(-1, 1, (7, n)).astype(F)
    want = mo.dct4_ref(u)
    _both(fft32, composed32, lambda f: _dct4_dev(f, u, in_place=True), want, f"dct4 N={n} in place")
    _both(fft32, composed32, lambda f: _dct4_dev(f, u, off=1), want, f"dct4 N={n} off=1")
    _both(fft32, composed32, lambda f: _dct4_dev(f, u, off=1, in_place=True), want, f"dct4 N={n} off=1 in place")
    assert bits_equal(km.dct4(u.reshape(7, 1, n), fft=fft32), want.reshape(7, 1, n))


@pytest.mark.parametrize("n", [64, 4096])
def test_dct4_off_alignment_takes_composed_route(fft32, oracle, n):
    """An input that is not 4-byte aligned: a byte view two bytes into its allocation."""
    import torch

    u = seeded(12300 + n).uniform(-1, 1, (3, n)).astype(F)
    raw = torch.zeros(u.nbytes + 8, dtype=torch.uint8, device="cuda")
    raw[2:2 + u.nbytes] = torch.from_numpy(u.reshape(-1).view(np.uint8)).cuda()
    out = torch.full((u.size,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # (the context's stream does not wait for torch's)
    fft32.dct4_fast_dev(raw.data_ptr() + 2, out.data_ptr(), n, 3)
    fft32.synchronize()
    assert_rows_equal(out.cpu().numpy().reshape(3, n), mo.dct4_ref(u), f"dct4 N={n} input off 4-byte alignment")


@pytest.mark.parametrize("n", [64, 2048, 240])
def test_dct4_special_values(fft32, composed32, oracle, n):
    tiny = np.array([1e-40, -1e-40, 1.4e-45], F)
    u = seeded(12400 + n).uniform(-1, 1, (6, n)).astype(F)
    u[0] = 0.0
    u[1] = -0.0
    u[2, :3] = tiny
    u[2, 3:] = 0.0
    u[3, 5] = np.inf
    u[4, n - 1] = -np.inf
    u[5, n // 2] = np.nan
    _both(fft32, composed32, lambda f: _dct4_dev(f, u), mo.dct4_ref(u), f"dct4 N={n} special values", nan_safe=True)


# ---- MDCT ------------------------------------------------------------------------------------------------------------------------------
def _mdct_case(fft32, composed32, n, rows, nx, lead, frames, stride, seed, host=True):
    x = seeded(seed).uniform(-1, 1, (rows, nx)).astype(F)
    w = seeded(seed + 1).uniform(0.1, 1, 2 * n).astype(F)
    want = mo.mdct_ref(x, w, lead, frames)
    what = f"mdct N={n} rows={rows} nx={nx} lead={lead} frames={frames} stride={stride}"
    _both(fft32, composed32, lambda f: _mdct_dev(f, x, w, lead, frames, stride), want, what + " dev")
    if host:
        _both(fft32, composed32, lambda f: _twice(lambda: f.mdct_rows(x, w, lead, frames), "mdct_rows"), want, what + " host")
    return want


@pytest.mark.parametrize("n", FUSED_N + COMPOSED_N)
def test_mdct_ladder(fft32, composed32, oracle, n):
    """3 rows x 5 frames: nx no multiple of N, the rows a stride apart with NaN between them, the last frame partly past the row's
    end.  3 x 5 items straddle the row seams inside a workgroup wherever XPB > 1 and leave the last workgroup partly empty."""
    nx = 3 * n + n // 2 + 1
    _mdct_case(fft32, composed32, n, 3, nx, n, 5, nx + 3, 12500 + n)


@pytest.mark.parametrize("n", [64, 512, 240])
def test_mdct_leads_and_frames_past_the_end(fft32, composed32, oracle, n):
    """lead 0, 1, N and 2N - 1; two frames wholly past the row's end, which are exactly zero."""
    nx = 2 * n + 5
    for lead in (0, 1, n, 2 * n - 1):
        frames = -(-(nx + lead) // n) + 2
        want = _mdct_case(fft32, composed32, n, 3, nx, lead, frames, nx + 1, 12600 + n + lead, host=(lead == n))
        assert not want[:, -2:].any()


def test_mdct_seam_inside_workgroups(fft32, composed32, oracle):
    """N = 64: 16 items per workgroup, 7 frames per row, 11 rows: every workgroup holds items of two or three rows."""
    _mdct_case(fft32, composed32, 64, 11, 300, 64, 7, 301, 12700)


def test_mdct_composed_across_scratch_seams(oracle, monkeypatch):
    """KOFFT_HIP_SCRATCH_CHUNK_MB=1 at N = 16384: 16 frames per chunk; 3 rows x 7 frames, so seams fall inside rows and row starts
    inside chunks."""
    import kofft_amd

    monkeypatch.setenv("KOFFT_HIP_SCRATCH_CHUNK_MB", "1")
    f = kofft_amd.HipFftImpl(F)
    try:
        n, rows, frames = 16384, 3, 7
        nx = 5 * n + 77
        x = seeded(12800).uniform(-1, 1, (rows, nx)).astype(F)
        w = _sine(n)
        want = mo.mdct_ref(x, w, n, frames)
        assert_rows_equal(_mdct_dev(f, x, w, n, frames, nx + 5).reshape(rows, -1), want.reshape(rows, -1), "mdct seams")
    finally:
        f.close()


# ---- IMDCT -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", FUSED_N + COMPOSED_N)
def test_imdct_ladder_and_windows(fft32, composed32, oracle, n):
    """3 rows x 5 frames; the whole of `full`, the signal's part, a window that starts and ends inside a block, one inside block 0."""
    rows, frames = 3, 5
    X = seeded(12900 + n).uniform(-1, 1, (rows, frames, n)).astype(F)
    w = seeded(12901 + n).uniform(0.1, 1, 2 * n).astype(F)
    scale = 2.0 / n
    full = mo.imdct_ref(X, w, scale)
    q = max(n // 4, 1)
    for first, count in [(0, (frames + 1) * n), (n, 4 * n - 1), (n + q, 2 * n + 1), (0, q), ((frames + 1) * n - 1, 1)]:
        want = np.ascontiguousarray(full[:, first:first + count])
        what = f"imdct N={n} window=({first}, {count})"
        _both(fft32, composed32, lambda f: _imdct_dev(f, X, w, scale, first, count), want, what + " dev")
        if first in (0, n):
            _both(fft32, composed32, lambda f: _twice(lambda: f.imdct_rows(X, w, scale, first, count), "imdct_rows"), want, what + " host")


@pytest.mark.parametrize("fused", [True, False])
def test_imdct_across_scratch_seams(oracle, monkeypatch, fused):
    """KOFFT_HIP_SCRATCH_CHUNK_MB=1 at N = 1024: 256 frames per chunk; 3 rows x 200 frames, so seams fall inside rows (a chunk
    recomputes the frame before its first) and row starts inside chunks.  Also a window that leaves out whole chunks."""
    import kofft_amd

    monkeypatch.setenv("KOFFT_HIP_SCRATCH_CHUNK_MB", "1")
    f = kofft_amd.HipFftImpl(F)
    try:
        f.set_mdct_fused(fused)
        n, rows, frames = 1024, 3, 200
        X = seeded(13000).uniform(-1, 1, (rows, frames, n)).astype(F)
        w = _sine(n)
        full = mo.imdct_ref(X, w, 2.0 / n)
        assert_rows_equal(_imdct_dev(f, X, w, 2.0 / n, 0, (frames + 1) * n), full, f"imdct seams fused={fused}")
        first, count = 57 * n + 100, 100 * n
        assert_rows_equal(_imdct_dev(f, X, w, 2.0 / n, first, count), np.ascontiguousarray(full[:, first:first + count]),
                          f"imdct seams window fused={fused}")
    finally:
        f.close()


# ---- both together -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 240, 1024, 8192])
def test_round_trip_on_the_device(fft32, composed32, oracle, n):
    """imdct(mdct(x)) against x within the bound measured on the CPU oracle (tests/test_mdct_cpu.py), through the module's functions
    with their defaults, for the three Princen-Bradley windows."""
    from kofft_amd import mdct as km

    x = seeded(13100 + n).uniform(-1, 1, (3, 5 * n + 3)).astype(F)
    for name, w in (("sine", None), ("vorbis", km.vorbis_window(n)), ("kbd", km.kbd_window(n))):
        for f in (fft32, composed32):
            X = km.mdct(x, n, window=w, fft=f)
            assert X.shape == (3, 7, n)
            back = km.imdct(X, window=w, length=x.shape[1], fft=f)
            err = rel(back, x)
            print(f"N={n} {name}: round trip relative L2 error {err:.3g}, bound {ROUND_TRIP[n]:.3g}")
            assert back.shape == x.shape and err <= ROUND_TRIP[n]
    one = km.imdct(km.mdct(x[0], n, fft=fft32), length=x.shape[1], fft=fft32)
    assert one.shape == (x.shape[1],) and rel(one, x[0]) <= ROUND_TRIP[n]


def test_python_errors(fft32):
    import kofft_amd

    E = kofft_amd.FftError
    x = np.ones((2, 100), F)
    w = np.ones(16, F)
    for call, code in [(lambda: fft32.mdct_rows(x, np.ones(15, F)), E.MismatchedLengths), (lambda: fft32.mdct_rows(x, w, lead=16), E.InvalidValue),
                       (lambda: fft32.mdct_rows(x, np.ones(14, F)), E.InvalidValue), (lambda: fft32.imdct_rows(np.ones((2, 3, 8), F), w, first=30, count=3), E.MismatchedLengths),
                       (lambda: fft32.dct4_fast_batch(np.ones((2, 5), F)), E.InvalidValue), (lambda: fft32.dct4_fast_batch(np.ones((2, 0), F)), E.EmptyInput)]:
        with pytest.raises(E) as e:
            call()
        assert e.value == E(code)
    assert fft32.mdct_rows(x, w, frames=0).shape == (2, 0, 8)
    assert fft32.imdct_rows(np.ones((2, 3, 8), F), w, count=0).shape == (2, 0)
    assert fft32.dct4_fast_batch(np.ones((0, 8), F)).shape == (0, 8)
