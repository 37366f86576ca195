"""The oracle's threaded entries (oracle/pyoracle.py: fft_mt, irfft_mt, rfft_mt, direct_mt) and the family oracles built on them give
the bytes of the serial entries, on batches that do not split evenly over the threads (no GPU)."""
import numpy as np
import pytest

from conftest import bits_equal, rand_c, seeded

RAGGED = [(1, 1), (5, 3), (17, 4), (100, 7), (33, 16)]  # (batch, threads): one row per thread, a short last block, more threads than rows


@pytest.mark.parametrize("cdt", [np.complex64, np.complex128])
@pytest.mark.parametrize("n", [1, 2, 12, 16, 1000, 4096])
def test_fft_mt_is_fft(oracle, cdt, n):
    for batch, threads in RAGGED:
        x = rand_c(seeded(20000 + n + batch), (batch, n), cdt)
        keep = x.copy()
        for inverse in (False, True):
            got = oracle.fft_mt(x, inverse=inverse, threads=threads)
            assert bits_equal(x, keep), "fft_mt copies: its input is left as it was"
            assert bits_equal(got, oracle.fft(x, inverse=inverse)), f"{cdt.__name__} n={n} batch={batch} inverse={inverse}"


def test_fft_mt_leading_axes_and_views(oracle):
    """Any leading axes are the batch, like the serial entry; a strided view is copied first."""
    x = rand_c(seeded(20100), (3, 5, 64))
    assert bits_equal(oracle.fft_mt(x, threads=4), oracle.fft(x))
    v = rand_c(seeded(20101), (40, 130))[::3, 1:65]
    assert bits_equal(oracle.fft_mt(v, inverse=True, threads=5), oracle.fft(v, inverse=True))


@pytest.mark.parametrize("rdt", [np.float32, np.float64])
@pytest.mark.parametrize("n", [2, 6, 10, 64, 1000, 4096, 1 << 15])
def test_irfft_mt_is_irfft(oracle, rdt, n):
    cdt = np.complex64 if rdt == np.float32 else np.complex128
    for batch, threads in RAGGED:
        spec = rand_c(seeded(20200 + n + batch), (batch, n // 2 + 1), cdt)
        spec[:, 0].imag = 0
        got = oracle.irfft_mt(spec, n, threads=threads)
        assert got.dtype == rdt and got.shape == (batch, n)
        assert bits_equal(got, oracle.irfft(spec, n)), f"{rdt.__name__} n={n} batch={batch}"


def test_threaded_entries_report_the_serial_errors(oracle):
    """An error of the C entry is raised on the calling thread, the one the serial entry raises."""
    with pytest.raises(oracle.OracleError) as e:  # an odd length
        oracle.irfft(np.zeros((5, 4), np.complex64), 7)
    with pytest.raises(oracle.OracleError) as e_mt:
        oracle.irfft_mt(np.zeros((5, 4), np.complex64), 7, threads=3)
    assert e.value.code == e_mt.value.code
    with pytest.raises(oracle.OracleError) as e:
        oracle.fft(np.zeros((2, 0), np.complex64))
    with pytest.raises(oracle.OracleError) as e_mt:
        oracle.fft_mt(np.zeros((2, 0), np.complex64))
    assert e.value.code == e_mt.value.code


def _family_rows(n, batch, seed):
    x = seeded(seed).uniform(-1, 1, (batch, n)).astype(np.float32)
    if n >= 4:
        x[0, 1] = np.inf
        x[1 % batch, 2] = np.nan
        x[-1, :] = np.float32(-0.0)
    return x


@pytest.mark.parametrize("n,batch", [(1, 9), (2, 5), (16, 37), (64, 1001), (4096, 19)])
def test_family_oracles_threaded_equal_serial(oracle, monkeypatch, n, batch):
    """dct2_ref, hilbert_ref and cepstrum_ref on the threaded entries give the bytes they give on the serial ones (NaNs included:
    the same x86 arithmetic on the same operands)."""
    from cepstrum_oracle import cepstrum_ref
    from dct_oracle import dct2_ref
    from hilbert_oracle import hilbert_ref

    x = _family_rows(n, batch, 20300 + n)
    threaded = [f(x) for f in (dct2_ref, hilbert_ref, cepstrum_ref)]
    monkeypatch.setattr(oracle, "fft_mt", lambda a, inverse=False, threads=None: oracle.fft(a, inverse))
    monkeypatch.setattr(oracle, "rfft_mt", lambda a, window=None, threads=None: oracle.rfft(a, window))
    serial = [f(x) for f in (dct2_ref, hilbert_ref, cepstrum_ref)]
    for name, a, b in zip(("dct2", "hilbert", "cepstrum"), threaded, serial):
        assert bits_equal(a, b), f"{name} n={n} batch={batch}"


@pytest.mark.parametrize("family,type", [(f, t) for f in ("dct", "dst") for t in (1, 2, 3, 4)])
def test_direct_mt_is_direct(oracle, family, type):
    """The cached table and the batch split over threads: the bytes of ko_direct_f32 (its own table, one thread)."""
    for n, batch, threads in [(1, 3, 2), (5, 17, 4), (257, 33, 7), (1000, 20, 16)]:
        x = seeded(20400 + n + type).uniform(-1, 1, (batch, n)).astype(np.float32)
        assert bits_equal(oracle.direct_mt(family, type, x, threads=threads), oracle.direct(family, type, x)), f"{family}{type} n={n}"
