"""tests/rowcheck.py's assert_rows_equal catches the faults a tiled or persistent kernel makes on a few rows of a large batch, and says
which rows (no GPU).  The first / middle / last sample that the device tests used before misses two of them."""
import numpy as np
import pytest

from conftest import bits_equal, rand_c, seeded
from rowcheck import assert_rows_equal, row_mismatches

BATCH, N = 1001, 24


def _want(dtype):
    rng = seeded(21000)
    if np.dtype(dtype).kind == "c":
        return rand_c(rng, (BATCH, N), dtype)
    return rng.uniform(-1, 1, (BATCH, N)).astype(dtype)


def _swap_interior(a):
    a[[400, 401]] = a[[401, 400]]
    return [400, 401]


def _zero_last(a):
    a[-1] = 0
    return [BATCH - 1]


def _one_ulp(a):
    v = a.view(a.real.dtype if a.dtype.kind == "c" else a.dtype).reshape(BATCH, -1)
    u = v.view({4: np.uint32, 8: np.uint64}[v.itemsize])
    u[733, 5] += 1
    return [733]


def _signed_zero(a):
    v = a.view(a.real.dtype if a.dtype.kind == "c" else a.dtype).reshape(BATCH, -1)
    v[250, 3] = 0.0
    return [250]


FAULTS = {"swap interior rows": _swap_interior, "zero the last row": _zero_last, "one ulp": _one_ulp, "+0 for -0": _signed_zero}


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.complex64, np.complex128])
@pytest.mark.parametrize("fault", list(FAULTS))
def test_planted_faults_are_caught_and_located(dtype, fault):
    want = _want(dtype)
    if fault == "+0 for -0":
        want.view(want.real.dtype if want.dtype.kind == "c" else want.dtype).reshape(BATCH, -1)[250, 3] = -0.0
    got = want.copy()
    rows = FAULTS[fault](got)
    assert_rows_equal(want.copy(), want, "unchanged")
    assert [r for r, _ in row_mismatches(got, want)] == rows
    with pytest.raises(AssertionError) as e:
        assert_rows_equal(got, want, fault)
    msg = str(e.value)
    assert f"{len(rows)} of {BATCH} rows differ" in msg and f"first at rows {rows}" in msg, msg
    assert f"row {rows[0]} col " in msg, msg


def test_the_old_sample_misses_the_interior_faults():
    """The {0, b/2, b-1} sample of the device tests sees the zeroed last row but not an interior swap or a one-ulp error; every row does."""
    want = _want(np.float32)
    sample = sorted({0, BATCH // 2, BATCH - 1})
    for fault, seen_by_sample in (("swap interior rows", False), ("one ulp", False), ("zero the last row", True)):
        got = want.copy()
        FAULTS[fault](got)
        assert bits_equal(got[sample], want[sample]) != seen_by_sample, fault
        with pytest.raises(AssertionError):
            assert_rows_equal(got, want, fault)


def test_report_names_the_first_differing_element():
    want = _want(np.complex64)
    got = want.copy()
    got[17, 9] = np.complex64(complex(want[17, 9].real, 2.5))
    got[900, 0] = np.complex64(complex(-1.0, want[900, 0].imag))
    with pytest.raises(AssertionError) as e:
        assert_rows_equal(got, want, "where")
    msg = str(e.value)
    assert "2 of 1001 rows differ, first at rows [17, 900]" in msg
    assert "row 17 col 9.im: got 2.5 (0x40200000)" in msg and "row 900 col 0.re: got -1.0 (0xbf800000)" in msg, msg


def test_nan_safe_moved_nan_and_nan_sign():
    """nan_safe: a NaN of the other sign in the same place is equal (the platform's default NaN differs between x86 and gfx950); a NaN
    moved to another element is not, nor is a NaN where the oracle has a number."""
    want = _want(np.float32)
    want[300, 4] = np.nan
    got = want.copy()
    got[300, 4] = -np.float32(np.nan)
    assert_rows_equal(got, want, "nan sign", nan_safe=True)
    with pytest.raises(AssertionError):
        assert_rows_equal(got, want, "nan sign, strict")
    moved = want.copy()
    moved[300, 4], moved[300, 5] = want[300, 5], np.nan
    with pytest.raises(AssertionError) as e:
        assert_rows_equal(moved, want, "moved nan", nan_safe=True)
    assert "1 of 1001 rows differ, first at rows [300]" in str(e.value) and "row 300 col 4" in str(e.value)
    cw = _want(np.complex64)
    cw[600, 2] = np.complex64(complex(np.nan, 1.0))
    cg = cw.copy()
    cg[600, 2] = np.complex64(complex(1.0, np.nan))
    with pytest.raises(AssertionError) as e:
        assert_rows_equal(cg, cw, "moved nan, complex", nan_safe=True)
    assert "row 600 col 2.re" in str(e.value)


def test_shape_and_dtype_mismatch_and_large_batches():
    want = _want(np.float32)
    with pytest.raises(AssertionError, match="shape|float32"):
        assert_rows_equal(want[:-1], want, "short")
    with pytest.raises(AssertionError, match="float64"):
        assert_rows_equal(want.astype(np.float64), want, "dtype")
    big = np.zeros((300_000, 64), np.float32)  # several comparison chunks: a fault in a later one is found and located
    got = big.copy()
    got[299_998, 63] = 1e-45
    with pytest.raises(AssertionError) as e:
        assert_rows_equal(got, big, "big")
    assert "first at rows [299998]" in str(e.value) and "row 299998 col 63" in str(e.value)
