"""Filter-bank overlap-save convolution / correlation of rows and the Morlet scalogram on it on the device, bit for
bit against tests/convolve_bank_oracle.py.  Blocks 32 .. 4096 run convolve_bank_fused_kernel<5 .. 12, kind> (one launch after the
filters' spectra: convolve_bank_filter_kernel, fft_dev); every other block -- and every block in a context with
set_convolve_bank_fused(False), or with x off 4-byte alignment -- runs convolve_expand_kernel -> fft_dev once per chunk, then per
filter convolve_bank_mul_kernel -> fft_dev(inverse) -> convolve_bank_gather_kernel<kind>.  The filter and gather kernels are the
one-filter family's too (test_gpu_convolve.py).  Every call runs twice and its two results are compared; the default context and the composed one get the same inputs and must give the same bytes."""
import numpy as np
import pytest

from conftest import bits_equal, seeded
from convolve_bank_oracle import KINDS, convolve_bank_ref
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32
XPB = {5: 32, 6: 16, 7: 16, 8: 16, 9: 4, 10: 4, 11: 2, 12: 1}  # items per workgroup of the fused kernel, by log2 block


@pytest.fixture(scope="module")
def composed32():
    """A context with the fused route off (set_convolve_bank_fused(False)): every bank through the composed route."""
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_convolve_bank_fused(False)
    yield f
    f.close()


def _rand(seed, rows, nx, filters, nh, cplx=False):
    rng = seeded(seed)
    x = rng.uniform(-1, 1, (rows, nx)).astype(F)
    h = rng.uniform(-1, 1, (filters, nh)).astype(F)
    if cplx:
        h = (h + 1j * rng.uniform(-1, 1, (filters, nh)).astype(F)).astype(np.complex64)
    return x, h


def _host(f, x, h, block, correlate=False, first=0, count=None, out="real"):
    a = f.convolve_bank_rows(x, h, block, correlate, first, count, out)
    b = f.convolve_bank_rows(x, h, block, correlate, first, count, out)
    assert bits_equal(a, b), "convolve_bank_rows: two runs of the same call differ"
    return a


def _dev(f, x, h, block, correlate=False, first=0, count=None, out="real", x_off=0):
    """The device entry on torch buffers, twice; x_off: bytes by which x is shifted into its allocation."""
    import torch

    rows, nx = x.shape
    filters, nh = h.shape
    cplx = h.dtype == np.complex64
    n_out = nx + nh - 1 - first if count is None else count
    per = 2 if out == "complex" else 1
    dx = torch.zeros(4 * x.size + 8, dtype=torch.uint8, device="cuda")
    dx[x_off:x_off + 4 * x.size] = torch.from_numpy(x.reshape(-1).view(np.uint8)).cuda()
    dh = torch.from_numpy(np.ascontiguousarray(h).reshape(-1).view(F)).cuda()
    res = []
    for _ in range(2):
        d_out = torch.full((rows * filters * n_out * per,), float("nan"), dtype=torch.float32, device="cuda")
        f.convolve_bank_dev(dx.data_ptr() + x_off, rows, nx, dh.data_ptr(), filters, nh, d_out.data_ptr(), block, correlate, first, n_out,
                            complex_taps=cplx, out=out)
        f.synchronize()
        got = d_out.cpu().numpy()
        res.append((got.view(np.complex64) if per == 2 else got).reshape(rows, filters, n_out))
    assert bits_equal(res[0], res[1]), "convolve_bank_dev: two runs of the same call differ"
    return res[0]


def _both(fft32, composed32, x, h, block, what, correlate=False, first=0, count=None, out="real", want=None, nan_safe=False, run=_host):
    if want is None:
        want = convolve_bank_ref(x, h, block, correlate, out)
    want = np.ascontiguousarray(want[:, :, first:None if count is None else first + count])
    got = run(fft32, x, h, block, correlate, first, count, out)
    assert_rows_equal(got, want, what + ": default route", nan_safe=nan_safe)
    got_c = run(composed32, x, h, block, correlate, first, count, out)
    assert_rows_equal(got_c, want, what + ": composed route", nan_safe=nan_safe)
    if not nan_safe:
        assert bits_equal(got, got_c), what + ": the two routes differ"


def _ladder_shape(log2b):
    """Five blocks per row (three from block 2048 on), the last one partial; more than one workgroup of the fused kernel with the
    last one partly empty, and workgroups whose items straddle a row seam."""
    block = 1 << log2b
    rows = 7 if block <= 256 else 3
    nh = block // 4 + 1
    hop = block - nh + 1
    nx = (2 if block >= 2048 else 4) * hop + 5
    if (nx + nh - 1) % hop == 0:
        nx += 1
    nb = -(-(nx + nh - 1) // hop)
    assert nb >= 3 and (nx + nh - 1) % hop != 0
    if XPB.get(log2b, 1) > 1:
        assert rows * nb % XPB[log2b] != 0 and rows * nb > XPB[log2b] and nb % XPB[log2b] != 0
    return block, rows, nx, nh


@pytest.mark.parametrize("log2b", range(1, 14))
def test_block_ladder(fft32, composed32, oracle, log2b):
    """Every block 2 .. 8192 with three real filters and the real part kept, through the host entry and the device entry."""
    block, rows, nx, nh = _ladder_shape(log2b)
    x, h = _rand(11300 + log2b, rows, nx, 3, nh)
    want = convolve_bank_ref(x, h, block)
    _both(fft32, composed32, x, h, block, f"block={block} rows={rows} nx={nx} nh={nh}", want=want)
    _both(fft32, composed32, x, h, block, f"block={block} rows={rows} nx={nx} nh={nh} dev", want=want, run=_dev)


@pytest.mark.parametrize("log2b", range(5, 13))
def test_complex_and_magnitude_on_every_fused_block(fft32, composed32, oracle, log2b):
    """The complex and the magnitude instance of the fused kernel at every block it has, on the ladder's shapes with complex taps."""
    block, rows, nx, nh = _ladder_shape(log2b)
    x, h = _rand(11400 + log2b, rows, nx, 2, nh, cplx=True)
    for out in ("complex", "magnitude"):
        _both(fft32, composed32, x, h, block, f"block={block} out={out}", out=out, run=_dev)


@pytest.mark.parametrize("correlate", [False, True])
@pytest.mark.parametrize("out", KINDS)
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("block", [64, 4096])
def test_tap_kinds_and_output_kinds(fft32, composed32, oracle, block, cplx, out, correlate):
    rows, nh = 3, block // 4 + 1
    nx = 2 * (block - nh + 1) + 5
    x, h = _rand(11500 + block + cplx, rows, nx, 3, nh, cplx)
    what = f"block={block} complex taps={cplx} out={out} correlate={correlate}"
    want = convolve_bank_ref(x, h, block, correlate, out)
    _both(fft32, composed32, x, h, block, what, correlate, out=out, want=want)
    _both(fft32, composed32, x, h, block, what + " dev", correlate, out=out, want=want, run=_dev)


@pytest.mark.parametrize("filters", [1, 2, 5])
def test_filter_counts(fft32, composed32, oracle, filters):
    x, h = _rand(11600 + filters, 5, 700, filters, 65, cplx=True)
    _both(fft32, composed32, x, h, 256, f"filters={filters}", out="complex")
    _both(fft32, composed32, x, h, 256, f"filters={filters} dev", out="magnitude", run=_dev)


@pytest.mark.parametrize("block", [16, 64, 4096, 8192])
def test_one_real_filter_is_the_one_filter_entry(fft32, composed32, block):
    """filters == 1, real taps, the real part: the bytes of kofft_hip_dev_convolve_f32 on the same buffers, on both routes of both."""
    import torch

    rows, nh = 3, block // 4 + 1
    nx = 2 * (block - nh + 1) + 5
    n_out = nx + nh - 1
    x, h = _rand(11700 + block, rows, nx, 1, nh)
    dx, dh = torch.from_numpy(x).cuda(), torch.from_numpy(h).cuda()
    for f in (fft32, composed32):
        one = torch.full((rows, n_out), float("nan"), device="cuda")
        bank = torch.full((rows, 1, n_out), float("nan"), device="cuda")
        f.convolve_dev(dx.data_ptr(), rows, nx, dh.data_ptr(), 1, nh, one.data_ptr(), block)
        f.convolve_bank_dev(dx.data_ptr(), rows, nx, dh.data_ptr(), 1, nh, bank.data_ptr(), block)
        f.synchronize()
        assert_rows_equal(bank.cpu().numpy()[:, 0], one.cpu().numpy(), f"block={block}")


def test_windows(fft32, composed32, oracle):
    """block 256, nh 65 (hop 192), nx 700: full 764 = 3 whole blocks + 188.  "same", "valid", a window inside one block, one from
    mid-block to mid-block, one sample, the last value only, the last partial block, the first sample, the whole, one whole block."""
    block, rows, nx, nh = 256, 5, 700, 65
    x, h = _rand(11800, rows, nx, 2, nh, cplx=True)
    want = {out: convolve_bank_ref(x, h, block, out=out) for out in KINDS}
    for first, count in [(32, 700), (64, 636), (200, 100), (100, 300), (391, 1), (763, 1), (600, 164), (0, 1), (0, 764), (192, 192),
                         (191, 194)]:
        for run, out in ((_host, "complex"), (_dev, "magnitude"), (_dev, "real")):
            _both(fft32, composed32, x, h, block, f"window first={first} count={count} {run.__name__} {out}", first=first, count=count,
                  out=out, want=want[out], run=run)


def test_edges(fft32, composed32, oracle):
    """Block 32: nh == block (hop 1), nh == 1 (hop == block, no leading zeros), nx < nh, one sample; and block 2 below every kernel."""
    for nx, nh, block in [(40, 32, 32), (1, 32, 32), (3 * 32 + 7, 1, 32), (5, 16, 32), (1, 1, 32), (7, 2, 2), (1, 1, 2)]:
        for rows in (1, 3):
            x, h = _rand(11900 + nx + nh, rows, nx, 2, nh, cplx=True)
            _both(fft32, composed32, x, h, block, f"block={block} rows={rows} nx={nx} nh={nh}", out="complex")
            _both(fft32, composed32, x, h, block, f"block={block} rows={rows} nx={nx} nh={nh} dev", True, out="real", run=_dev)


@pytest.mark.parametrize("rows,nx", [(4, 10000), (8, 100000)])
def test_host_equals_device(fft32, composed32, oracle, rows, nx):
    """The host entry and the device entry give the same bytes: 160 KB up and 480 KB down (zero-copy), 3.2 MB up and 9.6 MB down
    (staged), with the default block."""
    import kofft_amd

    nh = 100
    block = kofft_amd.convolve.default_block(nx, nh)
    assert block in (2048, 4096)  # (a fused block either way; which one is the library's measured choice)
    x, h = _rand(12000 + nx, rows, nx, 3, nh)
    want = convolve_bank_ref(x, h, block)
    for f in (fft32, composed32):
        got = _host(f, x, h, None)
        assert_rows_equal(got, want, f"host rows={rows} nx={nx}")
        assert bits_equal(got, _dev(f, x, h, None)), f"host against device rows={rows} nx={nx}"


@pytest.mark.parametrize("block", [64, 2048])
def test_x_off_four_byte_alignment_takes_the_composed_route(fft32, composed32, oracle, block):
    """x two bytes into its allocation: the default context sends the call through the composed route (plain 4-byte loads at any
    address), and the bytes are the aligned call's."""
    rows, nh = 3, block // 4 + 1
    nx = 2 * (block - nh + 1) + 5
    x, h = _rand(12100 + block, rows, nx, 2, nh, cplx=True)
    want = convolve_bank_ref(x, h, block, out="magnitude")
    for f, route in ((fft32, "default"), (composed32, "composed")):
        assert_rows_equal(_dev(f, x, h, block, out="magnitude", x_off=2), want, f"block={block} x off by two bytes, {route}")
        assert_rows_equal(_dev(f, x, h, block, out="magnitude", x_off=4), want, f"block={block} x off by four bytes, {route}")


def test_composed_route_across_scratch_seams(oracle, monkeypatch):
    """KOFFT_HIP_SCRATCH_CHUNK_MB=1: 64 items of 1024 points per chunk (a transformed frame and a product each); 3 rows of 60000
    samples at hop 768 are 79 frames each, so every seam falls inside a row."""
    import kofft_amd

    monkeypatch.setenv("KOFFT_HIP_SCRATCH_CHUNK_MB", "1")
    f = kofft_amd.HipFftImpl(F)
    try:
        f.set_convolve_bank_fused(False)
        x, h = _rand(12200, 3, 60000, 2, 257, cplx=True)
        want = convolve_bank_ref(x, h, 1024, out="complex")
        assert_rows_equal(_host(f, x, h, 1024, out="complex"), want, "seams")
        assert_rows_equal(_dev(f, x, h, 1024, first=1000, count=58000, out="complex"), want[:, :, 1000:59000], "seams window")
    finally:
        f.close()


@pytest.mark.parametrize("block", [64, 1024])
def test_special_values_stay_in_their_row(fft32, composed32, oracle, block):
    """A NaN in one block and Infs in others of row 1: NaNs come out exactly where the oracle has them, for every filter, everything
    else bit for bit; rows 0 and 2 are the bits of the clean signal."""
    rows, nh = 3, block // 4 + 1
    hop = block - nh + 1
    nx = 4 * hop + 5
    base, h = _rand(12300 + block, rows, nx, 2, nh, cplx=True)
    x = base.copy()
    x[1, 2 * hop + 1] = np.nan
    x[1, 0] = np.inf
    x[1, nx - 1] = -np.inf
    for out in ("real", "magnitude"):
        want = convolve_bank_ref(x, h, block, out=out)
        clean = convolve_bank_ref(base, h, block, out=out)
        assert np.isnan(want[1, :, 2 * hop:3 * hop]).all() and not np.isnan(want[1, :, hop:2 * hop]).any()
        assert bits_equal(want[0], clean[0]) and bits_equal(want[2], clean[2])
        _both(fft32, composed32, x, h, block, f"block={block} out={out} NaN and Inf samples", out=out, want=want, nan_safe=True, run=_dev)


def test_module_functions_and_modes(fft32, composed32, oracle):
    """kofft_amd.convolve.convolve_bank / correlate_bank: the three modes as windows of the full result, 1-D signals, an explicit
    block and the default one, real and complex banks."""
    from kofft_amd import convolve as cv

    x, h = _rand(12400, 3, 1000, 2, 33, cplx=True)
    hr = np.ascontiguousarray(h.real)
    for fn, corr in ((cv.convolve_bank, False), (cv.correlate_bank, True)):
        for block in (None, 64):
            b = block or 2048
            for taps, out in ((h, "complex"), (hr, "real"), (h, "magnitude")):
                want = convolve_bank_ref(x, taps, b, corr, out)
                for mode, first, count in [("full", 0, 1032), ("same", 16, 1000), ("valid", 32, 968)]:
                    for f in (fft32, composed32):
                        got = fn(x, taps, mode=mode, block=block, out=out, fft=f)
                        assert_rows_equal(got, np.ascontiguousarray(want[:, :, first:first + count]), f"{fn.__name__} {mode} block={b} {out}")
        got = fn(x[0], h, mode="same", out="complex", fft=fft32)
        assert got.shape == (2, 1000)
        assert_rows_equal(got, np.ascontiguousarray(convolve_bank_ref(x[:1], h, 2048, corr, "complex")[0, :, 16:1016]), f"{fn.__name__} 1-D")


def test_cwt_of_a_chirp(fft32, composed32):
    """kofft_amd.wavelet.cwt on two chirps of 3000 samples with six Morlet scales (nh 129, the default block 4096) against
    numpy.correlate(.., "same") in float64, inside convolve's bound at that block, for the complex values and the magnitudes; the
    caller's own taps through taps=; both routes the same bytes."""
    from kofft_amd import convolve as cv
    from kofft_amd import wavelet

    n = np.arange(3000)
    x = np.stack([np.cos(2 * np.pi * (0.01 + 0.00004 * n) * n), np.sin(2 * np.pi * (0.2 - 0.00003 * n) * n)]).astype(F)
    scales = 2.0 * 2.0 ** (np.arange(6) * 0.6)
    taps = wavelet.morlet_taps(scales)
    assert taps.shape == (6, 129) and cv.default_block(3000, 129) == 4096
    bound = 1e-6 + 2e-7 * 4096
    want = np.stack([[np.correlate(r.astype(np.float64), t.astype(np.complex128), "same") for t in taps] for r in x])
    got = wavelet.cwt(x, scales, out="complex", fft=fft32)
    mag = wavelet.cwt(x, scales, fft=fft32)
    assert got.shape == mag.shape == (2, 6, 3000) and got.dtype == np.complex64 and mag.dtype == F
    err_c = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    err_m = float(np.linalg.norm(mag - np.abs(want)) / np.linalg.norm(want))
    print(f"cwt: complex {err_c:.3g} magnitude {err_m:.3g} (bound {bound:.3g})")
    assert err_c <= bound and err_m <= bound
    assert bits_equal(mag, wavelet.cwt(x, taps=taps, fft=fft32)) and bits_equal(mag, wavelet.cwt(x, scales, fft=composed32))
    assert bits_equal(mag, cv.correlate_bank(x, taps, "same", out="magnitude", fft=fft32))
    assert wavelet.cwt(x[0], scales, fft=fft32).shape == (6, 3000)


def test_python_errors(fft32):
    import kofft_amd

    E = kofft_amd.FftError
    x = np.ones((2, 10), F)
    bank = np.ones((3, 5), F)
    for args, kw, code in [((x, bank), dict(block=4), E.MismatchedLengths), ((x, bank), dict(block=12), E.NonPowerOfTwoNoStd),
                           ((x, bank), dict(first=10, count=5), E.MismatchedLengths), ((x, np.ones((3, 0), F)), {}, E.EmptyInput)]:
        with pytest.raises(E) as e:
            fft32.convolve_bank_rows(*args, **kw)
        assert e.value == E(code)
    with pytest.raises(kofft_amd.DeviceError):
        fft32.convolve_bank_rows(x, bank, block=1 << 17)
    with pytest.raises(ValueError):
        fft32.convolve_bank_rows(x, bank, out="power")
    with pytest.raises(TypeError):
        fft32.convolve_bank_rows(x, np.ones(5, F))
    assert fft32.convolve_bank_rows(x, bank, count=0).shape == (2, 3, 0)
    assert fft32.convolve_bank_rows(np.ones((0, 10), F), bank).shape == (0, 3, 14)
    assert fft32.convolve_bank_rows(x, np.ones((0, 5), F)).shape == (2, 0, 14)
    got = fft32.convolve_bank_rows(x, np.ones((2, 1), F))  # block 16, nh 1: the composed route at its smallest
    assert got.shape == (2, 2, 10) and np.allclose(got, 1.0, atol=1e-6)
