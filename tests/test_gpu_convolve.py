"""Overlap-save convolution / correlation of rows on the device, bit for bit against tests/convolve_oracle.py.  Blocks
32 .. 4096 run convolve_fused_kernel<5 .. 12> (one launch after the filter's spectrum: convolve_bank_filter_kernel with real taps,
fft_dev); every other block -- and every block in a context with set_convolve_fused(False) -- runs convolve_expand_kernel -> fft_dev ->
convolve_mul_kernel -> fft_dev(inverse) -> convolve_bank_gather_kernel<BankReal> (one filter) through the context's scratch.  Every call runs twice and its two results are compared; the default context and
the composed one get the same inputs and must give the same bytes."""
import numpy as np
import pytest

from conftest import bits_equal, seeded
from convolve_oracle import convolve_ref
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32
XPB = {5: 32, 6: 16, 7: 16, 8: 16, 9: 4, 10: 4, 11: 2, 12: 1}  # items per workgroup of the fused kernel, by log2 block


@pytest.fixture(scope="module")
def composed32():
    """A context with the fused route off (set_convolve_fused(False)): every convolution through the composed route."""
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_convolve_fused(False)
    yield f
    f.close()


def _rand(seed, rows, nx, nh, per_row=False):
    rng = seeded(seed)
    return rng.uniform(-1, 1, (rows, nx)).astype(F), rng.uniform(-1, 1, (rows, nh) if per_row else nh).astype(F)


def _host(f, x, h, block, correlate=False, first=0, count=None):
    a = f.convolve_rows(x, h, block, correlate, first, count)
    b = f.convolve_rows(x, h, block, correlate, first, count)
    assert bits_equal(a, b), "convolve_rows: two runs of the same call differ"
    return a


def _dev(f, x, h, block, correlate=False, first=0, count=None, off=0):
    """The device entry on torch buffers, twice; off: floats by which x, h and the output are shifted into their allocations."""
    import torch

    rows, nx = x.shape
    nh = h.shape[-1]
    filters = 1 if h.ndim == 1 else h.shape[0]
    n_out = nx + nh - 1 - first if count is None else count
    dx = torch.zeros(x.size + off, dtype=torch.float32, device="cuda")
    dx[off:] = torch.from_numpy(x.reshape(-1)).cuda()
    dh = torch.zeros(h.size + off, dtype=torch.float32, device="cuda")
    dh[off:] = torch.from_numpy(h.reshape(-1)).cuda()
    res = []
    for _ in range(2):
        out = torch.full((rows * n_out + off,), float("nan"), dtype=torch.float32, device="cuda")
        f.convolve_dev(dx.data_ptr() + 4 * off, rows, nx, dh.data_ptr() + 4 * off, filters, nh, out.data_ptr() + 4 * off, block, correlate,
                       first, n_out)
        f.synchronize()
        res.append(out[off:].cpu().numpy().reshape(rows, n_out))
    assert bits_equal(res[0], res[1]), "convolve_dev: two runs of the same call differ"
    return res[0]


def _both(fft32, composed32, x, h, block, what, correlate=False, first=0, count=None, want=None, nan_safe=False, run=_host):
    if want is None:
        want = convolve_ref(x, h, block, correlate)
    want = np.ascontiguousarray(want[:, first:None if count is None else first + count])
    got = run(fft32, x, h, block, correlate, first, count)
    assert_rows_equal(got, want, what + ": default route", nan_safe=nan_safe)
    got_c = run(composed32, x, h, block, correlate, first, count)
    assert_rows_equal(got_c, want, what + ": composed route", nan_safe=nan_safe)
    if not nan_safe:
        assert bits_equal(got, got_c), what + ": the two routes differ"


@pytest.mark.parametrize("log2b", range(1, 14))
def test_block_ladder(fft32, composed32, oracle, log2b):
    """Every block 2 .. 8192 with five blocks per row, the last one partial, more than one workgroup of the fused kernel with the last
    one partly empty, and workgroups whose items straddle a row seam."""
    block = 1 << log2b
    rows = 11 if block <= 256 else 3
    nh = block // 4 + 1
    hop = block - nh + 1
    nx = 4 * hop + 5
    if (nx + nh - 1) % hop == 0:
        nx += 1
    nb = -(-(nx + nh - 1) // hop)
    assert nb >= 3 and (nx + nh - 1) % hop != 0
    if XPB.get(log2b, 1) > 1:
        assert rows * nb % XPB[log2b] != 0 and rows * nb > XPB[log2b] and nb % XPB[log2b] != 0
    x, h = _rand(9600 + log2b, rows, nx, nh)
    _both(fft32, composed32, x, h, block, f"block={block} rows={rows} nx={nx} nh={nh}")
    _both(fft32, composed32, x, h, block, f"block={block} rows={rows} nx={nx} nh={nh} dev", run=_dev)


@pytest.mark.parametrize("block", [32, 4096])
def test_edges(fft32, composed32, oracle, block):
    """nh == 1 (hop == block, no leading zeros), nh == block (hop 1; at 32), nx < nh, nx + nh - 1 == block exactly, each with one
    row and with three."""
    shapes = [(3 * block + 7, 1), (5, block // 2), (block - block // 4 + 1, block // 4), (1, 1)]
    if block == 32:
        shapes += [(40, block), (1, block)]
    for rows in (1, 3):
        for nx, nh in shapes:
            x, h = _rand(9700 + block + nx + nh, rows, nx, nh)
            _both(fft32, composed32, x, h, block, f"block={block} rows={rows} nx={nx} nh={nh}")


@pytest.mark.parametrize("correlate", [False, True])
@pytest.mark.parametrize("block", [64, 1024])
def test_per_row_filters_and_correlate(fft32, composed32, oracle, block, correlate):
    rows, nh = 5, block // 4 + 1
    nx = 3 * (block - nh + 1) + 5
    for per_row in (False, True):
        x, h = _rand(9800 + block + per_row, rows, nx, nh, per_row)
        what = f"block={block} per_row={per_row} correlate={correlate}"
        _both(fft32, composed32, x, h, block, what, correlate)
        _both(fft32, composed32, x, h, block, what + " dev", correlate, run=_dev)


def test_windows(fft32, composed32, oracle):
    """block 256, nh 65 (hop 192), nx 700: full 764 = 3 whole blocks + 188.  "same", "valid", a window from mid-block to mid-block,
    one sample, only the last partial block, the first sample, the whole."""
    block, rows, nx, nh = 256, 5, 700, 65
    x, h = _rand(9900, rows, nx, nh, per_row=True)
    want = convolve_ref(x, h, block)
    for first, count in [(32, 700), (64, 636), (100, 300), (391, 1), (600, 164), (763, 1), (0, 1), (0, 764), (192, 192), (191, 194)]:
        for run in (_host, _dev):
            _both(fft32, composed32, x, h, block, f"window first={first} count={count} {run.__name__}", first=first, count=count, want=want,
                  run=run)


@pytest.mark.parametrize("block", [64, 4096])
def test_unaligned_device_buffers(fft32, composed32, oracle, block):
    """Device buffers that are only 4-byte aligned (views one float into their allocations), on both routes."""
    rows, nh = 3, block // 4 + 1
    nx = 3 * (block - nh + 1) + 5
    x, h = _rand(10000 + block, rows, nx, nh)
    want = convolve_ref(x, h, block)
    for f, route in ((fft32, "default"), (composed32, "composed")):
        assert_rows_equal(_dev(f, x, h, block, off=1), want, f"block={block} unaligned {route}")


@pytest.mark.parametrize("rows,nx", [(8, 10000), (8, 200000)])
def test_host_equals_device(fft32, composed32, oracle, rows, nx):
    """The host entry and the device entry give the same bytes: 320 KB per direction (zero-copy) and 6.4 MB (staged), with the
    default block and per-row filters (a third staged array)."""
    import kofft_amd

    nh = 100
    block = kofft_amd.convolve.default_block(nx, nh)
    assert block in (2048, 4096)  # (a fused block either way; which one is the library's measured choice)
    for per_row in (False, True):
        x, h = _rand(10100 + nx + per_row, rows, nx, nh, per_row)
        want = convolve_ref(x, h, block)
        for f in (fft32, composed32):
            got = _host(f, x, h, None)
            assert_rows_equal(got, want, f"host rows={rows} nx={nx} per_row={per_row}")
            assert bits_equal(got, _dev(f, x, h, None)), f"host against device rows={rows} nx={nx} per_row={per_row}"


@pytest.mark.parametrize("per_row", [False, True])
def test_composed_route_across_scratch_seams(oracle, monkeypatch, per_row):
    """KOFFT_HIP_SCRATCH_CHUNK_MB=1: 128 frames of 1024 points per chunk; 5 rows of 60000 samples at hop 768 are 79 frames each
    (about 3 MB of frames in all), so every seam falls inside a row."""
    import kofft_amd

    monkeypatch.setenv("KOFFT_HIP_SCRATCH_CHUNK_MB", "1")
    f = kofft_amd.HipFftImpl(F)
    try:
        f.set_convolve_fused(False)
        x, h = _rand(10200 + per_row, 5, 60000, 257, per_row)
        want = convolve_ref(x, h, 1024)
        assert_rows_equal(_host(f, x, h, 1024), want, f"seams per_row={per_row}")
        assert_rows_equal(_dev(f, x, h, 1024, first=1000, count=58000), want[:, 1000:59000], f"seams window per_row={per_row}")
    finally:
        f.close()


@pytest.mark.parametrize("block", [32, 1024, 4096])
def test_special_values(fft32, composed32, oracle, block):
    """+-0, subnormals, +-Inf and NaN in x and in h: NaNs come out exactly where the oracle has them (a NaN or Inf sample poisons the
    blocks whose frames hold it and no other), everything else bit for bit."""
    rows, nh = 3, block // 4 + 1
    hop = block - nh + 1
    nx = 4 * hop + 5
    tiny = np.array([1e-40, -1e-40, 1.4e-45], F)
    base_x, base_h = _rand(10300 + block, rows, nx, nh)
    # zeros and subnormals: no NaN anywhere
    x = base_x.copy()
    x[0, :7] = [0.0, -0.0, *tiny, -0.0, 0.0]
    x[1] = -0.0
    x[2, hop:hop + 3] = tiny
    h = base_h.copy()
    h[:4] = [-0.0, tiny[0], 0.0, tiny[1]]
    _both(fft32, composed32, x, h, block, f"block={block} zeros and subnormals", nan_safe=True)
    # one NaN in block 2 of row 0, one Inf in block 0 of row 1 (past the overlap, so block 1 stays clean), -Inf in the last block of row 2
    x = base_x.copy()
    x[0, 2 * hop + 1] = np.nan
    x[1, 0] = np.inf
    x[2, nx - 1] = -np.inf
    want = convolve_ref(x, base_h, block)
    assert np.isnan(want[0, 2 * hop:3 * hop]).all() and not np.isnan(want[0, :hop]).any() and not np.isnan(want[0, 3 * hop:]).any()
    assert not np.isnan(want[1, hop:]).any() and not np.isnan(want[2, :3 * hop]).any()
    _both(fft32, composed32, x, base_h, block, f"block={block} NaN and Inf samples", want=want, nan_safe=True)
    # special taps: every block of every row meets them
    for tap in (np.nan, np.inf, -np.inf):
        h = base_h.copy()
        h[nh // 2] = tap
        _both(fft32, composed32, base_x, h, block, f"block={block} tap {tap}", nan_safe=True)


def test_module_functions_and_modes(fft32, composed32, oracle):
    """kofft_amd.convolve.convolve / correlate: the three modes as windows of the full result, 1-D inputs, per-row taps, an explicit
    block and the default one."""
    from kofft_amd import convolve as cv

    x, h = _rand(10400, 4, 1000, 33)
    _, hr = _rand(10401, 4, 1000, 33, per_row=True)
    for fn, corr in ((cv.convolve, False), (cv.correlate, True)):
        for block in (None, 64):
            b = block or cv.default_block(1000, 33)
            assert b == (block or 2048)
            for taps in (h, hr):
                want = convolve_ref(x, taps, b, corr)
                for mode, first, count in [("full", 0, 1032), ("same", 16, 1000), ("valid", 32, 968)]:
                    for f in (fft32, composed32):
                        got = fn(x, taps, mode=mode, block=block, fft=f)
                        assert_rows_equal(got, np.ascontiguousarray(want[:, first:first + count]), f"{fn.__name__} {mode} block={b}")
        got = fn(x[0], h, mode="same", fft=fft32)
        assert got.shape == (1000,)
        assert_rows_equal(got[None, :], np.ascontiguousarray(convolve_ref(x[:1], h, 2048, corr)[:, 16:1016]), f"{fn.__name__} 1-D")
    # against numpy in float64, to the oracle's bound at this block (tests/test_convolve_cpu.py)
    want64 = np.stack([np.correlate(r.astype(np.float64), h.astype(np.float64), "valid") for r in x])
    got = cv.correlate(x, h, mode="valid", fft=fft32)
    assert np.linalg.norm(got - want64) / np.linalg.norm(want64) <= 1e-6 + 2e-7 * 2048


def test_python_errors(fft32):
    import kofft_amd
    from kofft_amd import convolve as cv

    E = kofft_amd.FftError
    x = np.ones((2, 10), F)
    for args, kw, code in [((x, np.ones(5, F)), dict(block=4), E.MismatchedLengths), ((x, np.ones(5, F)), dict(block=12), E.NonPowerOfTwoNoStd),
                           ((x, np.ones((3, 5), F)), {}, E.MismatchedLengths), ((x, np.ones(5, F)), dict(first=10, count=5), E.MismatchedLengths),
                           ((x, np.ones(0, F)), {}, E.EmptyInput)]:
        with pytest.raises(E) as e:
            fft32.convolve_rows(*args, **kw)
        assert e.value == E(code)
    with pytest.raises(kofft_amd.DeviceError):
        fft32.convolve_rows(x, np.ones(5, F), block=1 << 17)
    assert fft32.convolve_rows(x, np.ones(5, F), count=0).shape == (2, 0)
    assert fft32.convolve_rows(np.ones((0, 10), F), np.ones(5, F)).shape == (0, 14)
    with pytest.raises(E) as e:
        cv.convolve(x, np.ones(11, F), mode="valid", fft=fft32)
    assert e.value == E(E.MismatchedLengths)
    got = cv.convolve(x, np.ones(1, F), fft=fft32)  # block 16, nh 1: the composed route at its smallest
    assert got.shape == (2, 10) and np.allclose(got, 1.0, atol=1e-6)
