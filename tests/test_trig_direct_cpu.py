"""The direct DCT-I..IV / DST-I..IV on the host side (no GPU): the test oracle against the float64 definitions, the library's tables
against the oracle's glibc tables bit for bit, the DstPlanner tables, the argument checks of the C ABI and of the Python modules, and
the machine code of the new kernels (nothing fused, no MFMA)."""
import ctypes as C
import re
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import seeded
from trig_direct_oracle import KINDS, direct, direct_f64, i_range, table

ROOT = Path(__file__).resolve().parent.parent
_libm = C.CDLL("libm.so.6")
_libm.sinf.restype = C.c_float
_libm.sinf.argtypes = [C.c_float]
_libm.sin.restype = C.c_double
_libm.sin.argtypes = [C.c_double]


@pytest.mark.parametrize("family,type", KINDS)
@pytest.mark.parametrize("n", [1, 2, 3, 8, 40, 256])
def test_oracle_is_the_transform(family, type, n):
    """The oracle's f32 sums agree with the float64 definitions within n * eps * sum |x * C| (plus the table's own rounding)."""
    x = seeded(9100 + 7 * n + type + (10 if family == "dst" else 0)).uniform(-1, 1, (3, n)).astype(np.float32)
    got = direct(family, type, x).astype(np.float64)
    want, mag = direct_f64(family, type, x)
    bound = (n + 4) * np.finfo(np.float32).eps * (mag + 1e-30) * 2
    assert np.all(np.abs(got - want) <= bound), f"{family}{type} n={n}: max err {np.max(np.abs(got - want) - bound)}"


def test_naive_dct2_agrees_with_plan_dct2(oracle):
    """dct.rs:183-195: the planner's DCT-II and the naive dct2 agree within 1e-4 on [1, 2, 3, 4]."""
    from dct_oracle import dct2_ref

    x = np.array([[1.0, 2.0, 3.0, 4.0]], np.float32)
    assert np.all(np.abs(direct("dct", 2, x) - dct2_ref(x)) < 1e-4)


def _lib_table(hiplib, family, type, n):
    c = np.empty((n, n), np.float32)
    fn = hiplib.kofft_hip_dct_direct_table_f32 if family == "dct" else hiplib.kofft_hip_dst_direct_table_f32
    assert fn(type, n, C.c_void_p(c.ctypes.data)) == 0
    return c


@pytest.mark.parametrize("family,type", KINDS)
@pytest.mark.parametrize("n", [1, 2, 3, 5, 40, 256])
def test_direct_table_is_glibc_bit_for_bit(hiplib, family, type, n):
    assert _lib_table(hiplib, family, type, n).tobytes() == table(family, type, n).tobytes()


@pytest.mark.parametrize("family,type", KINDS)
@pytest.mark.parametrize("n", [1024, 4095, 4096])
def test_direct_table_is_glibc_on_seeded_rows(hiplib, family, type, n):
    c = _lib_table(hiplib, family, type, n)
    rng = seeded(9300 + n + type)
    rows = sorted({0, 1, n - 2, n - 1} | set(rng.choice(n, 6, replace=False).tolist()))
    assert c[rows].tobytes() == table(family, type, n, rows=rows).tobytes()
    outside = [i for i in range(n) if i not in i_range(family, type, n)]
    assert not np.any(c[outside]), "rows outside the i range are +0"


@pytest.mark.parametrize("type", [2, 3, 4])
@pytest.mark.parametrize("n", [1, 2, 7, 64, 1000, 4096])
def test_dst_planner_tables(hiplib, type, n):
    """DstPlanner::build_table_offset (dst.rs:41-50): f32 through sinf, f64 through sin of (i as f32) as f64 + off as f64."""
    from kofft_amd.dst import DstPlanner

    off = 0.0 if type == 3 else 0.5
    i = np.arange(n, dtype=np.int64).astype(np.float32)
    a32 = (np.float32(np.pi) / np.float32(n)) * (i + np.float32(off))
    want32 = np.fromiter((_libm.sinf(float(v)) for v in a32), np.float32, n)
    a64 = (np.pi / float(np.float32(n))) * (i.astype(np.float64) + off)
    want64 = np.fromiter((_libm.sin(float(v)) for v in a64), np.float64, n)
    p32, p64 = DstPlanner(np.float32), DstPlanner(np.float64)
    plan = {2: "plan_dst2", 3: "plan_dst3", 4: "plan_dst4"}[type]
    assert getattr(p32, plan)(n).tobytes() == want32.tobytes()
    assert getattr(p64, plan)(n).tobytes() == want64.tobytes()
    assert getattr(p32, plan)(n) is getattr(p32, plan)(n)  # cached per length
    s = p32.scratch(5)
    assert s.shape == (5,) and s.dtype == np.float32 and not s.any()


def test_argument_checks_in_order_with_a_null_context(hiplib):
    """include/kofft_hip.h: type, batch == 0, n == 0 (EMPTY_INPUT for type 3), n > 4096, then null pointers -- no context needed."""
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    for stem in ("dct", "dst"):
        for fn in (getattr(hiplib, f"kofft_hip_{stem}_direct_f32"), getattr(hiplib, f"kofft_hip_{stem}_direct_f32_dev")):
            assert fn(None, 0, None, None, 0, 0) == 6  # INVALID_VALUE before everything
            assert fn(None, 5, p, p, 4, 1) == 6
            assert fn(None, 2, None, None, 4, 0) == 0  # batch == 0
            assert fn(None, 2, None, None, 0, 3) == 0  # n == 0: an empty result
            assert fn(None, 1, None, None, 0, 3) == 0
            assert fn(None, 3, None, None, 0, 3) == 1  # EMPTY_INPUT: input[0] indexed unchecked
            assert fn(None, 4, None, None, 4097, 1) == -2  # the table bound
            assert fn(None, 4, None, None, 4096, 1) == -3  # then the null context
            assert fn(None, 4, p, p, 4, 1) == -3
    for fn in (hiplib.kofft_hip_dct_direct_table_f32, hiplib.kofft_hip_dst_direct_table_f32):
        assert fn(0, 4, p) == 6 and fn(2, 0, None) == 0 and fn(2, 4097, p) == -2 and fn(2, 4, None) == -3
    for fn in (hiplib.kofft_hip_dst_planner_table_f32, hiplib.kofft_hip_dst_planner_table_f64):
        assert fn(1, 4, p) == 6 and fn(5, 4, p) == 6 and fn(2, 0, None) == 0 and fn(3, 4, None) == -3
    assert hiplib.kofft_hip_set_direct_tiled(None, 1) == -3


def test_python_errors_before_any_device():
    import kofft_amd
    from kofft_amd import api, dct, dst

    with pytest.raises(kofft_amd.FftError) as e:
        dct.dct3(np.zeros(0, np.float32))
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.EmptyInput)
    with pytest.raises(kofft_amd.FftError):
        dst.batch_iii([np.zeros(4, np.float32), np.zeros(0, np.float32)])
    with pytest.raises(kofft_amd.DeviceError):
        dst.dst2(np.zeros((2, 4097), np.float32))
    with pytest.raises(kofft_amd.DeviceError):
        dct.batch_i([np.zeros(3, np.float32), np.zeros(5000, np.float32)])
    with pytest.raises(TypeError):
        dct.dct1(np.zeros((1, 2, 3), np.float32))
    with pytest.raises(TypeError):
        dct.batch_ii([np.zeros(4, np.float64)])
    with pytest.raises(kofft_amd.FftError):
        api.direct_transform("dct", 5, np.zeros(4, np.float32))
    assert dct.dct1(np.zeros(0, np.float32)).shape == (0,)
    assert dst.dst4(np.zeros((3, 0), np.float32)).shape == (3, 0)
    rows = [np.zeros(0, np.float32)]
    dct.batch_ii(rows)  # only empty rows: nothing to run
    assert api._direct_default is None, "a context was created before the errors"


LIB = ROOT / "kofft_amd" / "lib" / "libkofft_hip.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")


@pytest.mark.skipif(not LIB.exists() or not (LLVM / "llvm-objdump").exists(), reason="needs the built library and ROCm's llvm-objdump")
def test_direct_kernels_have_no_fused_or_mfma_instruction():
    """-ffp-contract=off and the kernels' own arithmetic: every term is one multiply and one add (dct.rs / dst.rs do not fuse)."""
    sys.path.insert(0, str(ROOT / "tools"))
    from check_store_hazard import disassemble

    funcs = {}
    for _, listing in disassemble(LIB):
        for func, lines in _functions(listing):
            if "direct_tiled_kernel" in func or "direct_simple_kernel" in func:
                funcs[func] = lines
    assert len(funcs) == 6, sorted(funcs)
    bad = re.compile(r"^\s*(v_fma\w*|v_pk_fma\w*|v_fmac\w*|v_mac_\w*|v_mad_f32|v_mad_legacy\w*|v_mfma\w*|v_dot\w*)\b")
    for func, lines in funcs.items():
        hits = [ln for ln in lines if bad.match(ln)]
        assert not hits, f"{func}: {hits[:3]}"
    for func, lines in funcs.items():
        if "tiled" in func:
            assert sum("v_pk_mul_f32" in ln for ln in lines) >= 512 and sum("v_pk_add_f32" in ln for ln in lines) >= 512, func


def _functions(listing):
    """(name, lines) per function of one code object's disassembly."""
    out, cur, lines = [], None, []
    for item in listing:
        m = re.match(r"^[0-9a-f]+ <(.*)>:", item)
        if m:
            if cur:
                out.append((cur, lines))
            cur, lines = m.group(1), []
        elif cur:
            lines.append(item)
    if cur:
        out.append((cur, lines))
    return out


def _c_oracle_rows(n, rng):
    """Random rows, rows of one special value, and random rows with specials planted: +-0, subnormals, +-Inf, NaN, 3e38."""
    specials = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1.2e-38, np.inf, -np.inf, np.nan, 3e38, -3e38], np.float32)
    rows = [rng.uniform(-1, 1, n).astype(np.float32) for _ in range(3)]
    rows += [np.full(n, v, np.float32) for v in (-0.0, 0.0, 3e38, 1e-40)]
    for j in range(len(specials)):
        r = rng.uniform(-1, 1, n).astype(np.float32)
        r[rng.choice(n, size=min(n, 1 + j % 3), replace=False)] = specials[j]
        rows.append(r)
    rows.append(specials[rng.integers(0, len(specials), n)])
    return np.stack(rows)


@pytest.mark.parametrize("family,type", KINDS)
@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 257, 1000, 4096])
def test_c_oracle_is_the_numpy_restatement(oracle, family, type, n):
    """oracle/kofft_oracle.c's ko_direct_f32 (the all-rows, all-columns oracle of the device tests beyond n = 256) is a second
    transcription of the reference's loops: the bytes of trig_direct_oracle.direct, NaNs included, on every column up to n = 257 and
    on seeded columns (both ends and every 128-column tile edge) beyond."""
    from trig_direct_oracle import sample_cols

    x = _c_oracle_rows(n, seeded(9700 + n + 10 * type + (5 if family == "dst" else 0)))
    got = oracle.direct(family, type, x)
    cols = None if n <= 257 else sample_cols(n, 24, 9800 + n)
    want = direct(family, type, x, cols)
    assert (got if cols is None else got[:, cols]).tobytes() == want.tobytes(), f"{family}{type} n={n}"
    assert oracle.direct_mt(family, type, x, threads=5).tobytes() == got.tobytes()
    assert oracle.direct_table(family, type, n)[:, cols or slice(None)].tobytes() == table(family, type, n, None, cols).tobytes()
