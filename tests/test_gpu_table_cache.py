"""The table cache (kofft_amd/csrc/host_cache.h) as "build, then hit, then a second context", for the kinds no other test takes through
that sequence: the Bluestein pair (chirp + fft(b)), the radix-4 pair (permutation + triples), stft_magnitudes' Hann window and the
DCT-II (cos, sin) table.  Every call runs twice on a fresh context -- the first builds the tables, the second finds them -- and again
on a second context, which has to build its own; every row is the oracle's bits.  Then release_scratch: the tables stay, the
Bluestein work buffer is allocated again, the bytes are the same."""
import numpy as np
import pytest

from conftest import rand_c, seeded
from dct_oracle import dct2_ref
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu

BLUE_N, BLUE_BATCH = 100, 3  # m = 256: the one-launch arm; KOFFT_HIP_BLUESTEIN_ONE=0 contexts loop over the work buffer
R4_N, R4_BATCH = 64, 5
MAG_LEN, MAG_WIN, MAG_HOP = 1000, 64, 16
DCT_N, DCT_BATCH = 100, 3
CDT = {np.float32: np.complex64, np.float64: np.complex128}


@pytest.fixture(scope="module")
def cases(oracle):
    """Inputs and the oracle's outputs, computed once and never written to."""
    c = {}
    for dt, cdt in CDT.items():
        xb = rand_c(seeded(4100 + cdt().itemsize), (BLUE_BATCH, BLUE_N), cdt)
        xr = rand_c(seeded(4200 + cdt().itemsize), (R4_BATCH, R4_N), cdt)
        c[dt] = dict(blue=xb, blue_fwd=oracle.fft(xb), blue_inv=oracle.ifft(xb), r4=xr, r4_fwd=oracle.fft_radix4(xr))
    sig = seeded(4300).uniform(-1, 1, MAG_LEN).astype(np.float32)
    c["mag"] = (sig,) + tuple(oracle.stft_magnitudes(sig, MAG_WIN, MAG_HOP))
    rows = seeded(4400).uniform(-1, 1, (DCT_BATCH, DCT_N)).astype(np.float32)
    c["dct"] = (rows, dct2_ref(rows))
    for v in c.values():
        for a in (v.values() if isinstance(v, dict) else v):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return c


def _bluestein(f, case, what):
    for inverse, want in ((False, case["blue_fwd"]), (True, case["blue_inv"])):
        y = case["blue"].copy()
        f.fft_batch(y, inverse=inverse)
        assert_rows_equal(y, want, f"{what} bluestein n={BLUE_N} inverse={inverse}")


def _every_kind(f, dt, cases, what):
    _bluestein(f, cases[dt], what)
    y = cases[dt]["r4"].copy()
    f.fft_radix4_batch(y)
    assert_rows_equal(y, cases[dt]["r4_fwd"], f"{what} fft_radix4 n={R4_N}")
    if dt == np.float32:
        sig, want, want_max = cases["mag"]
        mags, mx = f.stft_magnitudes(sig, MAG_WIN, MAG_HOP)
        assert_rows_equal(mags, want, f"{what} stft_magnitudes")
        assert mx == want_max, what
        rows, want = cases["dct"]
        assert_rows_equal(f.dct2_batch(rows), want, f"{what} dct2 n={DCT_N}")


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["c32", "c64"])
def test_tables_build_then_hit_on_two_contexts(cases, dt, monkeypatch):
    import kofft_amd as K

    for name in ("first", "second"):
        f = K.HipFftImpl(dt)
        try:
            for call in ("build", "hit"):
                _every_kind(f, dt, cases, f"{name} context, {call}")
            f.release_scratch()  # the tables survive, the scratch does not
            _bluestein(f, cases[dt], f"{name} context, after release_scratch")
        finally:
            f.close()
    # ... and with the Bluestein arm on its work buffer (blue_tmp), which release_scratch frees and the next call allocates again
    monkeypatch.setenv("KOFFT_HIP_BLUESTEIN_ONE", "0")
    f = K.HipFftImpl(dt)
    try:
        for what in ("build", "hit"):
            _bluestein(f, cases[dt], f"work-buffer context, {what}")
        f.release_scratch()
        _bluestein(f, cases[dt], "work-buffer context, after release_scratch")
    finally:
        f.close()
