"""hilbert::hilbert_analytic (hilbert.rs:13-47) on the device, bit for bit against tests/hilbert_oracle.py.  Powers of two 32 .. 4096
run hilbert_fused_kernel<5 .. 12> (one launch); every other length -- and every length in a context with set_hilbert_fused(False) --
runs expand_real_kernel -> fft_dev (in place) -> hilbert_mask_kernel -> fft_dev(inverse), whose batch ladders are there for
fft_dev's routes: the one-thread kernels, the workgroup kernel, every persistent-kernel threshold of the n-point transform (host_common.hip.h:
dispatch; the per-CU factors are restated below, as test_gpu_dct.py does), the register-file kernel at 2^15 and the factor path above."""
import numpy as np
import pytest

from conftest import bits_equal, seeded
from hilbert_oracle import hilbert_ref
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def num_cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _persist_rows(log2n, cus):
    """Smallest batch at which dispatch() runs the persistent form of the f32 n-point transform (None: it has none)."""
    per_cu = {6: 512, 7: 256, 8: 128, 9: 64, 10: 32, 11: 16, 12: 4, 13: 4, 14: 4}.get(log2n)
    return None if per_cu is None else per_cu * cus


def _twice(f, x):
    """hilbert_batch twice on the same input: the two results must be the same bytes."""
    a = f.hilbert_batch(x)
    b = f.hilbert_batch(x)
    assert bits_equal(a, b), "hilbert_batch: two runs of the same call differ"
    return a


def _check(f, x, what=""):
    got = _twice(f, x)
    assert got.dtype == np.complex64 and got.shape == x.shape, what
    assert_rows_equal(got, hilbert_ref(x), what)


@pytest.fixture(scope="module")
def composed32():
    """A context with the fused route off (set_hilbert_fused(False)): every analytic signal through the composed route."""
    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    f.set_hilbert_fused(False)
    return f


@pytest.mark.parametrize("log2n", range(0, 21))
def test_hilbert_pow2_batch_ladder(fft32, oracle, num_cus, log2n):
    """n = 1 .. 2^20 at batches 1, 3, 257 (2^15 and above: 1, 3), at the persistent threshold (+1) of the n-point transform and, at
    2^15, at the register-file kernel's threshold (CUs x 2)."""
    n = 1 << log2n
    batches = [1, 3, 257] if log2n <= 14 else [1, 3]
    p = _persist_rows(log2n, num_cus)
    if p is not None:
        batches.append(p + 1)
    if log2n == 15:
        batches.append(2 * num_cus + 1)
    for batch in batches:
        x = seeded(7100 + 37 * log2n + batch).uniform(-1, 1, (batch, n)).astype(np.float32)
        _check(fft32, x, what=f"n={n} batch={batch}")


@pytest.mark.parametrize("log2n", range(0, 15))
def test_hilbert_fused_equals_composed(fft32, composed32, oracle, num_cus, log2n):
    """The fused kernel (n = 32 .. 4096) and the composed route give the same bytes, at batches that leave the fused kernel's last
    workgroup partly empty (it takes 256 / (n >> rl_for) rows: 32, 16, 16, 16, 4, 4, 2, 1) and at the n-point transform's persistent
    threshold, which the composed route reaches."""
    n = 1 << log2n
    p = _persist_rows(log2n, num_cus)
    for batch in [1, 5, 33] + ([p + 1] if p is not None else []):
        x = seeded(7200 + 41 * log2n + batch).uniform(-1, 1, (batch, n)).astype(np.float32)
        fused = _twice(fft32, x)
        composed = _twice(composed32, x)
        assert bits_equal(fused, composed), f"n={n} batch={batch}"
        assert_rows_equal(fused, hilbert_ref(x), f"n={n} batch={batch}")


def test_hilbert_unaligned_device_rows(fft32, composed32, oracle):
    """A device input that is only 4-byte aligned (a view one float into an allocation): the same bytes as the oracle, on both routes."""
    import torch

    for n, batch in [(1024, 7), (64, 40), (4096, 3), (8, 5), (8192, 3)]:
        x = seeded(7600 + n).uniform(-1, 1, (batch, n)).astype(np.float32)
        d = torch.empty(batch * n + 1, dtype=torch.float32, device="cuda")
        d[1:] = torch.from_numpy(x.reshape(-1)).cuda()
        want = hilbert_ref(x)
        for f in (fft32, composed32):
            d_out = torch.empty((batch, n), dtype=torch.complex64, device="cuda")
            f.hilbert_dev(d.data_ptr() + 4, d_out.data_ptr(), n, batch)
            f.synchronize()
            assert bits_equal(d_out.cpu().numpy(), want), f"n={n} batch={batch}"


def test_hilbert_host_equals_dev(fft32, oracle, monkeypatch):
    """The host entry point and the device-pointer entry point give the same bytes: zero-copy, staged, and (in a context with the
    host pipeline on) a batch of 200 MB in + out that goes up and down in eight chunks."""
    import torch
    import kofft_amd

    monkeypatch.setenv("KOFFT_HIP_HOST_PIPELINE", "1")  # read when the context is created
    piped = kofft_amd.HipFftImpl(np.float32)
    for f, n, batch in [(fft32, 8, 5), (fft32, 1024, 300), (fft32, 65536, 3), (piped, 4096, 4096 + 5), (piped, 16, (1 << 20) + 3)]:
        x = seeded(7700 + n).uniform(-1, 1, (batch, n)).astype(np.float32)
        host = f.hilbert_batch(x)
        d_in = torch.from_numpy(x).cuda()
        d_out = torch.empty((batch, n), dtype=torch.complex64, device="cuda")
        f.hilbert_dev(d_in.data_ptr(), d_out.data_ptr(), n, batch)
        f.synchronize()
        assert bits_equal(d_out.cpu().numpy(), host), f"n={n} batch={batch}"
        assert_rows_equal(host, hilbert_ref(x), f"n={n} batch={batch}")


def test_hilbert_analytic_free_function(oracle):
    """The module-level hilbert_analytic: a 1-D signal gives n complex64 values; a 2-D input one row per row."""
    import kofft_amd

    x = seeded(7800).uniform(-1, 1, (3, 256)).astype(np.float32)
    want = hilbert_ref(x)
    one = kofft_amd.hilbert_analytic(x[1])
    assert one.shape == (256,) and bits_equal(one, want[1])
    assert bits_equal(kofft_amd.hilbert_analytic(x), want)
    assert bits_equal(kofft_amd.hilbert_analytic(list(x[2][:16])), hilbert_ref(x[2:3, :16])[0])


def test_hilbert_errors(fft32, fft64):
    """n = 0 -> EmptyInput, n not a power of two -> NonPowerOfTwoNoStd (hilbert.rs:14-19), n beyond 2^26 -> KOFFT_ERR_UNSUPPORTED, batch 0 ->
    nothing to do; f64 contexts and 1-D arrays are refused by hilbert_batch."""
    import kofft_amd

    with pytest.raises(kofft_amd.FftError) as e:
        fft32.hilbert_batch(np.zeros((2, 0), np.float32))
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.EmptyInput)
    for n in (3, 12, 4095):
        with pytest.raises(kofft_amd.FftError) as e:
            fft32.hilbert_batch(np.zeros((2, n), np.float32))
        assert e.value == kofft_amd.FftError(kofft_amd.FftError.NonPowerOfTwoNoStd)
    with pytest.raises(kofft_amd.FftError) as e:
        kofft_amd.hilbert_analytic(np.zeros(6, np.float32), fft32)
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.NonPowerOfTwoNoStd)
    with pytest.raises(kofft_amd.DeviceError) as d:
        fft32.hilbert_dev(0, 0, 1 << 27, 1)
    assert d.value.code == -2  # KOFFT_ERR_UNSUPPORTED
    assert fft32.hilbert_dev(0, 0, 8, 0) is None
    with pytest.raises(TypeError):
        fft64.hilbert_batch(np.zeros((1, 8), np.float64))
    with pytest.raises(TypeError):
        fft32.hilbert_batch(np.zeros(8, np.float32))


@pytest.mark.parametrize("n", [1, 2, 8, 64, 1024, 4096, 1 << 16])
def test_hilbert_special_values(fft32, composed32, oracle, n):
    """+-0, subnormals, +-Inf and NaN go through the same operations as in the reference -- the mask's two real multiplies keep an Inf
    an Inf -- on both routes: NaNs in the same places, every other value (-0.0 and subnormal outputs included) the same bits."""
    specials = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, np.inf, -np.inf, np.nan, 1.0, -3.5], np.float32)
    rng = seeded(7900 + n)
    rows = []
    for i in range(len(specials) + 2):
        r = rng.uniform(-1, 1, n).astype(np.float32)
        if i < len(specials):
            r[rng.integers(0, n)] = specials[i]
        elif i == len(specials):
            r[:] = specials[rng.integers(0, len(specials), n)]
        else:
            r[:] = np.float32(-0.0)
        rows.append(r)
    x = np.stack(rows)
    want = hilbert_ref(x)
    assert np.isnan(want.view(np.float32)).any()
    for f in (fft32, composed32):
        got = _twice(f, x)
        assert_rows_equal(got, want, f"n={n}", nan_safe=True)
