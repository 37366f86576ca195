"""DctPlanner::plan_dct2 on the host side (no GPU): the library's (cos, sin) table against glibc, the test oracle's DCT-II
against the textbook transform, and the planner's argument checks."""
import ctypes as C

import numpy as np
import pytest

from conftest import seeded
from dct_oracle import cos_sin, dct2_f64, dct2_ref


@pytest.mark.parametrize("n", [1, 2, 3, 40, 1024, 4096, 1 << 20])
def test_dct2_table_matches_glibc_bit_for_bit(hiplib, n):
    """kofft_hip_dct2_table_f32: cosf / sinf of PI * k / (2n) in f32 (dct.rs:54, 90-91), the same bits as glibc's own calls."""
    cs = np.empty((n, 2), np.float32)
    assert hiplib.kofft_hip_dct2_table_f32(n, C.c_void_p(cs.ctypes.data)) == 0
    c, s = cos_sin(n)
    assert cs[:, 0].tobytes() == c.tobytes(), f"cos n={n}"
    assert cs[:, 1].tobytes() == s.tobytes(), f"sin n={n}"


def test_dct2_table_null_pointer(hiplib):
    assert hiplib.kofft_hip_dct2_table_f32(4, None) == -3  # KOFFT_ERR_NULL
    assert hiplib.kofft_hip_dct2_table_f32(0, None) == 0


def test_planner_cos_table_is_the_library_table():
    import kofft_amd

    p = kofft_amd.DctPlanner()
    assert p.get_cos_table(40).tobytes() == cos_sin(40)[0].tobytes()
    assert p.get_cos_table(40) is p.get_cos_table(40)  # cached per length, as dct.rs:50-58


@pytest.mark.parametrize("n", [1, 2, 3, 8, 40, 1024])
def test_dct2_ref_is_the_dct2(oracle, n):
    """The composition (oracle rfft of the mirrored row, f32 twist) is the DCT-II to f32 rounding."""
    x = seeded(4100 + n).uniform(-1, 1, (3, n)).astype(np.float32)
    got = dct2_ref(x).astype(np.float64)
    want = dct2_f64(x)
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    assert err <= 2e-6 * max(1.0, np.log2(n)), f"n={n} rel_err={err:.2e}"


def test_planner_rejects_mismatched_lengths_without_a_device():
    """dct.rs:68-70: output.len() != input.len() -> MismatchedLengths, checked before anything runs (no context is created)."""
    import kofft_amd

    p = kofft_amd.DctPlanner()
    run = p.plan_dct2(8)
    for x, y in [(np.zeros(8, np.float32), np.zeros(7, np.float32)),
                 (np.zeros(8, np.float32), np.zeros(9, np.float32)),
                 (np.zeros((2, 8), np.float32), np.zeros((2, 7), np.float32)),
                 (np.zeros(6, np.float32), np.zeros(6, np.float32))]:  # rows not of the planned length
        with pytest.raises(kofft_amd.FftError) as e:
            run(x, y)
        assert e.value == kofft_amd.FftError(kofft_amd.FftError.MismatchedLengths)
    with pytest.raises(kofft_amd.FftError) as e:
        p.plan_dct2(0)(np.zeros(0, np.float32), np.zeros(0, np.float32))
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.EmptyInput)
    assert p._impl is None
