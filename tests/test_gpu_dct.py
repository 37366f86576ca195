"""DctPlanner::plan_dct2 (dct.rs:61-105) on the device, bit for bit against tests/dct_oracle.py (the oracle's rfft of the mirrored
rows, then the f32 twist).  Powers of two 32 .. 4096 run dct2_fused_kernel<5 .. 12> (one launch); every other length -- and every
length in a context with set_dct_fused(False) -- runs dct2_mirror_kernel -> fft_dev (n-point, in place) -> dct2_post_kernel, whose
batch ladders are there for fft_dev's routes: the one-thread kernels, the workgroup kernel and every persistent-kernel threshold of
the n-point transform (host_common.hip.h: dispatch; the per-CU factors are restated below, as test_gpu_route_coverage.py restates
the factor path's), computed from the device's CU count."""
import numpy as np
import pytest

from conftest import bits_equal, seeded
from dct_oracle import dct2_ref
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


def _dct_twice(f, x):
    """dct2_batch twice on the same input: the two results must be the same bytes (the session fixture does not wrap it)."""
    a = f.dct2_batch(x)
    b = f.dct2_batch(x)
    assert bits_equal(a, b), "dct2_batch: two runs of the same call differ"
    return a


def _check(f, x, what=""):
    """Every row against the oracle."""
    assert_rows_equal(_dct_twice(f, x), dct2_ref(x), what)


@pytest.mark.parametrize("log2n", range(0, 15))
def test_dct2_pow2_batch_ladder(fft32, oracle, num_cus, log2n):
    """n = 1 .. 2^14 at batches 1, 3, 257 and at the persistent kernel's threshold (+1) of the n-point transform."""
    n = 1 << log2n
    batches = [1, 3, 257]
    p = _persist_rows(log2n, num_cus)
    if p is not None:
        batches.append(p + 1)
    for batch in batches:
        x = seeded(6100 + 37 * log2n + batch).uniform(-1, 1, (batch, n)).astype(np.float32)
        _check(fft32, x, what=f"n={n} batch={batch}")


@pytest.fixture(scope="module")
def composed32():
    """A context with the fused route off (set_dct_fused(False)): every DCT-II through the composed route."""
    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    f.set_dct_fused(False)
    return f


@pytest.mark.parametrize("log2n", range(0, 15))
def test_dct2_fused_equals_composed(fft32, composed32, oracle, num_cus, log2n):
    """The fused kernel (n = 32 .. 4096) and the composed route give the same bytes, at batches that leave a partial last workgroup
    (the fused kernel takes 512 / n rows per workgroup below n = 512) and at the n-point transform's persistent threshold."""
    n = 1 << log2n
    p = _persist_rows(log2n, num_cus)
    for batch in [1, 5, 33] + ([p + 1] if p is not None else []):
        x = seeded(6200 + 41 * log2n + batch).uniform(-1, 1, (batch, n)).astype(np.float32)
        fused = _dct_twice(fft32, x)
        composed = _dct_twice(composed32, x)
        assert bits_equal(fused, composed), f"n={n} batch={batch}"
        assert_rows_equal(fused, dct2_ref(x), f"n={n} batch={batch}")


def test_dct2_unaligned_device_rows(fft32, oracle):
    """A device input that is only 4-byte aligned (a view one float into an allocation) takes the composed route with 4-byte loads:
    the same bytes as an aligned input."""
    import torch

    for n, batch in [(1024, 7), (64, 40), (100, 3)]:
        x = seeded(6600 + n).uniform(-1, 1, (batch, n)).astype(np.float32)
        d = torch.empty(batch * n + 1, dtype=torch.float32, device="cuda")
        d[1:] = torch.from_numpy(x.reshape(-1)).cuda()
        d_out = torch.empty((batch, n), dtype=torch.float32, device="cuda")
        fft32.dct2_dev(d.data_ptr() + 4, d_out.data_ptr(), n, batch)
        fft32.synchronize()
        assert bits_equal(d_out.cpu().numpy(), dct2_ref(x)), f"n={n} batch={batch}"


@pytest.mark.parametrize("log2n", range(15, 21))
def test_dct2_large_pow2(fft32, oracle, num_cus, log2n):
    """n = 2^15 .. 2^20: the factor path (and the register-file kernel at 2^15 from CUs x 2 transforms); every row."""
    n = 1 << log2n
    batches = [3] + ([2 * num_cus + 1] if log2n == 15 else [])
    for batch in batches:
        x = seeded(6300 + log2n + batch).uniform(-1, 1, (batch, n)).astype(np.float32)
        _check(fft32, x, what=f"n={n} batch={batch}")


@pytest.mark.parametrize("n", [3, 5, 12, 40, 100, 1000, 4095])
def test_dct2_non_pow2(fft32, oracle, n):
    """Lengths whose n-point transform is Bluestein's (dct.rs:86 -> rfft.rs:447 -> fft.rs:1083-1132)."""
    for batch in (1, 17):
        x = seeded(6500 + n + batch).uniform(-1, 1, (batch, n)).astype(np.float32)
        _check(fft32, x, what=f"n={n} batch={batch}")


def test_dct2_host_equals_dev(fft32, oracle, monkeypatch):
    """The host entry point and the device-pointer entry point give the same bytes: zero-copy (400 KiB each way at n = 1024, batch
    100: the per-direction limit), staged, and (in a context with the host pipeline on) a batch of 128 MiB each way that goes up
    and down in eight chunks."""
    import torch
    import kofft_amd

    monkeypatch.setenv("KOFFT_HIP_HOST_PIPELINE", "1")  # read when the context is created
    piped = kofft_amd.HipFftImpl(np.float32)
    cases = [(fft32, 8, 5), (fft32, 1024, 100), (fft32, 1024, 300), (fft32, 100, 70), (fft32, 4096, 20000), (piped, 4096, 8192 + 5)]
    for f, n, batch in cases:
        x = seeded(6700 + n).uniform(-1, 1, (batch, n)).astype(np.float32)
        host = f.dct2_batch(x)
        d_in = torch.from_numpy(x).cuda()
        d_out = torch.empty_like(d_in)
        f.dct2_dev(d_in.data_ptr(), d_out.data_ptr(), n, batch)
        f.synchronize()
        assert bits_equal(d_out.cpu().numpy(), host), f"n={n} batch={batch}"
        assert_rows_equal(host, dct2_ref(x), f"n={n} batch={batch}")
    piped.close()


def test_dct2_planner(oracle):
    """DctPlanner.plan_dct2: one row, a batch of rows, and a planner on an explicit HipFftImpl."""
    import kofft_amd

    x = seeded(6800).uniform(-1, 1, (6, 40)).astype(np.float32)
    want = dct2_ref(x)
    run = kofft_amd.DctPlanner().plan_dct2(40)
    out = np.empty(40, np.float32)
    run(x[2], out)
    assert bits_equal(out, want[2])
    outs = np.empty_like(x)
    kofft_amd.DctPlanner(kofft_amd.HipFftImpl(np.float32)).plan_dct2(40)(x, outs)
    assert bits_equal(outs, want)


def test_dct2_errors(fft32):
    """n = 0 -> EmptyInput (rfft.rs:434); an output of the wrong length -> MismatchedLengths (dct.rs:68-70); n beyond the
    complex transform's range -> KOFFT_ERR_UNSUPPORTED, before any pointer is touched."""
    import kofft_amd

    with pytest.raises(kofft_amd.FftError) as e:
        fft32.dct2_batch(np.zeros((2, 0), np.float32))
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.EmptyInput)
    run = kofft_amd.DctPlanner(fft32).plan_dct2(16)
    with pytest.raises(kofft_amd.FftError) as e:
        run(np.zeros(16, np.float32), np.zeros(15, np.float32))
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.MismatchedLengths)
    for n in ((1 << 25) + 1, 1 << 27):
        with pytest.raises(kofft_amd.DeviceError) as d:
            fft32.dct2_dev(0, 0, n, 1)
        assert d.value.code == -2  # KOFFT_ERR_UNSUPPORTED
    assert fft32.dct2_dev(0, 0, 8, 0) is None  # batch 0: nothing to do


@pytest.mark.parametrize("n", [1, 8, 100, 1024, 1 << 16])
def test_dct2_special_values(fft32, oracle, n):
    """+-0, subnormals, +-Inf and NaN go through the same operations as in the reference: NaNs in the same places, every other value
    (-0.0 and subnormal outputs included) the same bits."""
    specials = np.array([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, np.inf, -np.inf, np.nan, 1.0, -3.5], np.float32)
    rng = seeded(6900 + n)
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
    got = _dct_twice(fft32, x)
    want = dct2_ref(x)
    assert np.isnan(want).any()
    assert_rows_equal(got, want, f"n={n}", nan_safe=True)
