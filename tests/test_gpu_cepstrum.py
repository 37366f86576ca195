"""cepstrum::real_cepstrum (cepstrum.rs:12-33) on the device, bit for bit against tests/cepstrum_oracle.py.  Powers of two 32 .. 4096 run
cepstrum_fused_kernel<5 .. 12> (one launch); every other length -- and every length in a context with set_cepstrum_fused(False) -- runs
expand_real_kernel -> fft_dev (in place, in the context's scratch) -> cepstrum_logmag_kernel -> fft_dev(inverse) -> cepstrum_real_kernel,
whose batch ladders are there for fft_dev's routes: the one-thread kernels, the workgroup kernel, every persistent-kernel threshold of the
n-point transform (host_common.hip.h: dispatch; the per-CU factors are restated below, as test_gpu_hilbert.py does), the register-file
kernel at 2^15 and the factor path above.  The libm crate's logf (libm_logf.hip.h) has no entry point of its own: the cepstra of these
random rows reach it in every bin, and tools/ubench_logf.hip checks it on every f32."""
import numpy as np
import pytest

from cepstrum_oracle import cepstrum_ref
from conftest import bits_equal, seeded
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
    """cepstrum_batch twice on the same input: the two results must be the same bytes."""
    a = f.cepstrum_batch(x)
    b = f.cepstrum_batch(x)
    assert bits_equal(a, b), "cepstrum_batch: two runs of the same call differ"
    return a


def _check(f, x, what=""):
    got = _twice(f, x)
    assert got.dtype == np.float32 and got.shape == x.shape, what
    assert_rows_equal(got, cepstrum_ref(x), what)


@pytest.fixture(scope="module")
def composed32():
    """A context with the fused route off (set_cepstrum_fused(False)): every real cepstrum through the composed route."""
    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    f.set_cepstrum_fused(False)
    return f


@pytest.mark.parametrize("log2n", range(0, 21))
def test_cepstrum_pow2_batch_ladder(fft32, oracle, num_cus, log2n):
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
        x = seeded(8100 + 37 * log2n + batch).uniform(-1, 1, (batch, n)).astype(np.float32)
        _check(fft32, x, what=f"n={n} batch={batch}")


@pytest.mark.parametrize("log2n", range(0, 15))
def test_cepstrum_fused_equals_composed(fft32, composed32, oracle, num_cus, log2n):
    """The fused kernel (n = 32 .. 4096) and the composed route give the same bytes, at batches that leave the fused kernel's last
    workgroup partly empty (it takes 256 / (n >> rl_for) rows: 32, 16, 16, 16, 4, 4, 2, 1) and at the n-point transform's persistent
    threshold, which the composed route reaches."""
    n = 1 << log2n
    p = _persist_rows(log2n, num_cus)
    for batch in [1, 5, 33] + ([p + 1] if p is not None else []):
        x = seeded(8200 + 41 * log2n + batch).uniform(-1, 1, (batch, n)).astype(np.float32)
        fused = _twice(fft32, x)
        composed = _twice(composed32, x)
        assert bits_equal(fused, composed), f"n={n} batch={batch}"
        assert_rows_equal(fused, cepstrum_ref(x), f"n={n} batch={batch}")


def test_cepstrum_unaligned_device_rows(fft32, composed32, oracle):
    """A device input that is only 4-byte aligned (a view one float into an allocation), and an output likewise: the same bytes as the
    oracle, on both routes."""
    import torch

    for n, batch in [(1024, 7), (64, 40), (4096, 3), (8, 5), (8192, 3)]:
        x = seeded(8600 + n).uniform(-1, 1, (batch, n)).astype(np.float32)
        d = torch.empty(batch * n + 1, dtype=torch.float32, device="cuda")
        d[1:] = torch.from_numpy(x.reshape(-1)).cuda()
        want = cepstrum_ref(x)
        for f in (fft32, composed32):
            d_out = torch.empty(batch * n + 1, dtype=torch.float32, device="cuda")
            f.cepstrum_dev(d.data_ptr() + 4, d_out.data_ptr() + 4, n, batch)
            f.synchronize()
            assert bits_equal(d_out[1:].cpu().numpy().reshape(batch, n), want), f"n={n} batch={batch}"


def test_cepstrum_in_place(fft32, composed32, oracle):
    """in == out on both routes (every route reads all of a row before it writes any of it): the oracle's bytes.  The composed route's
    scratch is cut into row chunks of 512 MiB: 2^20 + 5 rows of 64 take two of them."""
    import torch

    for n, batch in [(1, 9), (16, 100), (64, (1 << 20) + 5), (256, 77), (4096, 33), (8192, 5), (1 << 17, 3)]:
        x = seeded(8650 + n).uniform(-1, 1, (batch, n)).astype(np.float32)
        want = cepstrum_ref(x)
        for f in (fft32, composed32):
            d = torch.from_numpy(x).cuda()
            f.cepstrum_dev(d.data_ptr(), d.data_ptr(), n, batch)
            f.synchronize()
            assert_rows_equal(d.cpu().numpy(), want, f"n={n} batch={batch}")


def test_cepstrum_host_equals_dev(fft32, oracle, monkeypatch):
    """The host entry point and the device-pointer entry point give the same bytes: zero-copy, staged, and (in a context with the
    host pipeline on) batches of 128 MiB in + out that go up and down in eight chunks."""
    import torch
    import kofft_amd

    monkeypatch.setenv("KOFFT_HIP_HOST_PIPELINE", "1")  # read when the context is created
    piped = kofft_amd.HipFftImpl(np.float32)
    for f, n, batch in [(fft32, 8, 5), (fft32, 1024, 30), (fft32, 1024, 300), (fft32, 65536, 3), (piped, 4096, 4096 + 5),
                        (piped, 1024, 16384 + 3), (piped, 16, (1 << 20) + 3)]:
        x = seeded(8700 + n + batch).uniform(-1, 1, (batch, n)).astype(np.float32)
        host = f.cepstrum_batch(x)
        d_in = torch.from_numpy(x).cuda()
        d_out = torch.empty((batch, n), dtype=torch.float32, device="cuda")
        f.cepstrum_dev(d_in.data_ptr(), d_out.data_ptr(), n, batch)
        f.synchronize()
        assert bits_equal(d_out.cpu().numpy(), host), f"n={n} batch={batch}"
        assert_rows_equal(host, cepstrum_ref(x), f"n={n} batch={batch}")


def test_real_cepstrum_free_function(oracle):
    """The module-level real_cepstrum: a 1-D signal gives n float32 values; a 2-D input one row per row."""
    import kofft_amd

    x = seeded(8800).uniform(-1, 1, (3, 256)).astype(np.float32)
    want = cepstrum_ref(x)
    one = kofft_amd.real_cepstrum(x[1])
    assert one.shape == (256,) and one.dtype == np.float32 and bits_equal(one, want[1])
    assert bits_equal(kofft_amd.real_cepstrum(x), want)
    assert bits_equal(kofft_amd.real_cepstrum(list(x[2][:16])), cepstrum_ref(x[2:3, :16])[0])
    # the reference's own test input (cepstrum.rs tests): [1, 2, 3, 4]
    four = np.array([1.0, 2.0, 3.0, 4.0], np.float32)
    assert bits_equal(kofft_amd.real_cepstrum(four), cepstrum_ref(four[None, :])[0])


def test_cepstrum_errors(fft32, fft64):
    """n = 0 -> EmptyInput, n not a power of two -> NonPowerOfTwoNoStd (cepstrum.rs:13-18), n beyond 2^26 -> KOFFT_ERR_UNSUPPORTED,
    batch 0 -> nothing to do; f64 contexts and 1-D arrays are refused by cepstrum_batch."""
    import kofft_amd

    with pytest.raises(kofft_amd.FftError) as e:
        fft32.cepstrum_batch(np.zeros((2, 0), np.float32))
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.EmptyInput)
    for n in (3, 12, 4095):
        with pytest.raises(kofft_amd.FftError) as e:
            fft32.cepstrum_batch(np.zeros((2, n), np.float32))
        assert e.value == kofft_amd.FftError(kofft_amd.FftError.NonPowerOfTwoNoStd)
    with pytest.raises(kofft_amd.FftError) as e:
        kofft_amd.real_cepstrum(np.zeros(6, np.float32), fft32)
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.NonPowerOfTwoNoStd)
    with pytest.raises(kofft_amd.DeviceError) as d:
        fft32.cepstrum_dev(0, 0, 1 << 27, 1)
    assert d.value.code == -2  # KOFFT_ERR_UNSUPPORTED
    assert fft32.cepstrum_dev(0, 0, 8, 0) is None
    with pytest.raises(TypeError):
        fft64.cepstrum_batch(np.zeros((1, 8), np.float64))
    with pytest.raises(TypeError):
        fft32.cepstrum_batch(np.zeros(8, np.float32))


@pytest.mark.parametrize("n", [1, 2, 8, 64, 1024, 4096, 1 << 16])
def test_cepstrum_special_values(fft32, composed32, oracle, n):
    """Rows that reach every arm of the pointwise step, on both routes: +-0 rows (every bin logs 1e-12), subnormal rows, rows near
    3e38 and 1e20 (re * re overflows to inf although |X| is finite: log = inf), and +-Inf / NaN samples.  NaNs in the same places,
    every other value (-0.0 and subnormal outputs included) the same bits."""
    rng = seeded(8900 + n)
    rows = [np.zeros(n, np.float32), np.full(n, -0.0, np.float32),
            rng.choice(np.array([1e-45, -1e-45, 1e-40, -3e-39, 1.1754942e-38, 0.0], np.float32), n),
            (rng.uniform(0.5, 1.0, n) * 3e38).astype(np.float32), (rng.uniform(-1, 1, n) * 1e20).astype(np.float32),
            (rng.uniform(-1, 1, n) * 2e19).astype(np.float32)]
    for special in (np.inf, -np.inf, np.nan):
        r = rng.uniform(-1, 1, n).astype(np.float32)
        r[rng.integers(0, n)] = special
        rows.append(r)
    r = np.zeros(n, np.float32)
    r[0] = np.float32(1e-30)  # |X| = 1e-30 in every bin: re * re underflows to 0
    rows.append(r)
    x = np.stack(rows)
    want = cepstrum_ref(x)
    assert np.isnan(want).any() and np.isfinite(want).any()
    for f in (fft32, composed32):
        got = _twice(f, x)
        assert_rows_equal(got, want, f"n={n}", nan_safe=True)
