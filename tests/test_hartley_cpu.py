"""The Hartley transform on the host side (no GPU): the library's restated sinf / cosf (kofft_amd/csrc/libm_trigf.hip.h, compiled for
the host) against the numpy restatement of tests/hartley_oracle.py bit for bit and against the correctly rounded value, the table, the
reference's own pins, the argument checks, the machine code of dht_table_kernel and the host table code under sanitizers."""
import ctypes as C
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import hartley_oracle as ho
from conftest import bits_equal, seeded

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
ANGLE_NS = (2, 3, 5, 64, 1000, 4096)


def _lib_trig(hiplib, x):
    x = np.ascontiguousarray(x, F)
    c, s = np.empty(x.shape, F), np.empty(x.shape, F)
    rc = hiplib.kofft_hip_libm_trigf(C.c_void_p(x.ctypes.data), x.size, C.c_void_p(c.ctypes.data), C.c_void_p(s.ctypes.data))
    assert rc == 0, rc
    return c, s


def _bounds():
    """Each branch bound of sinf.rs / cosf.rs and the last pattern of rem_pio2f's medium range, with the patterns one below and one
    above (below only at the end of the range), both signs."""
    pats = [b + d for b in ho.BOUNDS for d in (-1, 0, 1)] + [ho.MEDIUM_END - 2, ho.MEDIUM_END - 1]
    u = np.array(pats, np.uint32)
    return np.concatenate([u, u | np.uint32(0x80000000)]).view(F)


@pytest.fixture(scope="module")
def trig_sets(hiplib):
    """name -> (x, library cos, library sin, oracle cos, oracle sin), every finite input set of the issue, computed once."""
    sets = {}
    for n in ANGLE_NS:  # every angle of the table: the distinct values of factor * (i * k) as f32
        sets[f"n={n}"] = np.unique(ho.angles(n))
    rng = seeded(20100)
    sets["random"] = (rng.uniform(0, 25800, 1 << 20) * rng.choice([-1.0, 1.0], 1 << 20)).astype(F)
    sets["bounds"] = _bounds()
    sets["small"] = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, 1.2e-38, 2.0 ** -13, -(2.0 ** -13)], F)
    out = {}
    for name, x in sets.items():
        lc, ls = _lib_trig(hiplib, x)
        out[name] = (x, lc, ls, ho.cosf(x), ho.sinf(x))
    return out


def test_libm_trigf_equals_the_numpy_restatement_bit_for_bit(hiplib, trig_sets):
    for name, (x, lc, ls, oc, os_) in trig_sets.items():
        assert bits_equal(lc, oc), f"cosf {name}: {int(np.sum(lc.view(np.uint32) != oc.view(np.uint32)))} of {x.size} differ"
        assert bits_equal(ls, os_), f"sinf {name}: {int(np.sum(ls.view(np.uint32) != os_.view(np.uint32)))} of {x.size} differ"
    x = np.array([np.inf, -np.inf, np.nan], F)
    lc, ls = _lib_trig(hiplib, x)
    assert np.isnan(lc).all() and np.isnan(ls).all() and np.isnan(ho.cosf(x)).all() and np.isnan(ho.sinf(x)).all()
    z = np.array([0.0, -0.0], F)
    lc, ls = _lib_trig(hiplib, z)
    assert bits_equal(ls, z) and bits_equal(lc, np.ones(2, F)), "sinf keeps the sign of zero, cosf(0) is 1"


def _ordered(a):
    """float32 -> integers in which neighbouring floats differ by one."""
    i = a.view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def test_both_restatements_are_within_one_ulp_and_mostly_correctly_rounded(trig_sets):
    """Against np.cos / np.sin in float64 rounded to f32: never more than 1 ulp off, equal in at least 99.9 % of the finite inputs
    (the published error of the kernels is 2^-37.5: a mistyped coefficient or branch constant shows here, not in the bit-for-bit
    test, which both restatements could pass wrong together).  Found: 99.95 % or more, lowest at n = 64."""
    total = {"cos": [0, 0], "sin": [0, 0]}
    for name, (x, lc, ls, oc, os_) in trig_sets.items():
        x64 = x.astype(np.float64)
        for what, want, got_all in (("cos", np.cos(x64).astype(F), (lc, oc)), ("sin", np.sin(x64).astype(F), (ls, os_))):
            for who, got in zip(("library", "oracle"), got_all):
                ulp = np.abs(_ordered(got) - _ordered(want))
                worst = int(ulp.max())
                share = float(np.mean(ulp == 0))
                print(f"{what} {name} {who}: {x.size} inputs, worst {worst} ulp, correctly rounded {100 * share:.4f} %")
                assert worst <= 1, f"{what} {name} {who}: {worst} ulp at x = {x[int(ulp.argmax())]!r}"
                if who == "library":
                    total[what][0] += int(np.sum(ulp == 0))
                    total[what][1] += x.size
    for what, (hit, cnt) in total.items():
        print(f"{what}: correctly rounded {100 * hit / cnt:.4f} % of {cnt}")
        assert hit >= 0.999 * cnt, f"{what}: only {100 * hit / cnt:.4f} % correctly rounded"


def test_libm_trigf_refuses_what_needs_rem_pio2_large(hiplib):
    for pat in (ho.MEDIUM_END, ho.MEDIUM_END | 0x80000000, 0x7f7fffff):
        x = np.array([1.0, 0.0], F)
        x.view(np.uint32)[1] = pat
        c = np.full(2, 7.0, F)
        s = np.full(2, 7.0, F)
        rc = hiplib.kofft_hip_libm_trigf(C.c_void_p(x.ctypes.data), 2, C.c_void_p(c.ctypes.data), C.c_void_p(s.ctypes.data))
        assert rc == -2 and np.all(c == 7.0) and np.all(s == 7.0), hex(pat)
        with pytest.raises(ValueError):
            ho.sinf(x)
    p = C.c_void_p(np.zeros(1, F).ctypes.data)
    assert hiplib.kofft_hip_libm_trigf(None, 0, None, None) == 0
    assert hiplib.kofft_hip_libm_trigf(None, 1, p, p) == -3 and hiplib.kofft_hip_libm_trigf(p, 1, None, p) == -3


def _lib_table(hiplib, n):
    h = np.empty((n, n), F)
    assert hiplib.kofft_hip_dht_table_f32(n, C.c_void_p(h.ctypes.data)) == 0
    return h


@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 129, 1000])
def test_table_is_the_oracles_and_symmetric(hiplib, n):
    h = _lib_table(hiplib, n)
    assert bits_equal(h, ho.table(n))
    assert bits_equal(h, np.ascontiguousarray(h.T)), "H[i][k] depends on i * k only"
    assert bits_equal(h[0], np.ones(n, F)) and bits_equal(h[:, 0], np.ones(n, F)), "cosf(0) + sinf(0) = 1"


def test_the_references_own_pins(hiplib):
    """hartley.rs:63-70, 102-125, on the oracle's sums over the library's table (the device runs the same in tests/test_gpu_hartley.py)."""
    x = np.array([[1.0, 2.0, 3.0, 4.0]], F)
    for h in (ho.table(4), _lib_table(hiplib, 4)):
        z = ho.dht(ho.dht(x, h), h)
        assert np.all(np.abs(x - z / F(4.0)) < 1e-5), z
    assert bits_equal(ho.dht(np.zeros((1, 8), F), _lib_table(hiplib, 8)), np.zeros((1, 8), F))
    ones = ho.dht(np.ones((1, 8), F), _lib_table(hiplib, 8))
    assert np.any(np.abs(ones) > 0)
    assert ho.dht(np.zeros((1, 0), F)).shape == (1, 0)
    one = ho.dht(np.array([[1.0]], F), _lib_table(hiplib, 1))
    assert one.shape == (1, 1) and one[0, 0] == 1.0


def test_argument_checks_in_order_with_a_null_context(hiplib):
    """include/kofft_hip.h: batch == 0, n == 0, n > 4096, then null pointers -- no context needed."""
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    for fn in (hiplib.kofft_hip_dht_f32, hiplib.kofft_hip_dev_dht_f32):
        assert fn(None, None, None, 4097, 0) == 0  # batch == 0 before everything
        assert fn(None, None, None, 0, 3) == 0     # n == 0: an empty result
        assert fn(None, None, None, 4097, 1) == -2  # the table bound before the pointers
        assert fn(None, p, p, 4097, 1) == -2
        assert fn(None, None, None, 4096, 1) == -3  # then the null context
        assert fn(None, p, p, 4, 1) == -3
    assert hiplib.kofft_hip_set_dht_table_device(None, 1) == -3
    t = hiplib.kofft_hip_dht_table_f32
    assert t(0, None) == 0 and t(4097, p) == -2 and t(4, None) == -3


def test_python_errors_before_any_device():
    import kofft_amd
    from kofft_amd import api, hartley

    before = api._direct_default
    with pytest.raises(kofft_amd.DeviceError):
        hartley.dht(np.zeros((2, 4097), F))
    with pytest.raises(kofft_amd.DeviceError):
        hartley.batch([np.zeros(3, F), np.zeros(5000, F)])
    with pytest.raises(TypeError):
        hartley.dht(np.zeros((1, 2, 3), F))
    with pytest.raises(TypeError):
        hartley.batch([np.zeros(4, np.float64)])
    assert hartley.dht(np.zeros(0, F)).shape == (0,)
    assert hartley.dht(np.zeros((3, 0), F)).shape == (3, 0)
    hartley.multi_channel([np.zeros(0, F)])  # only empty rows: nothing to run
    assert api._direct_default is before, "a context was created before the errors"


LIB = ROOT / "kofft_amd" / "lib" / "libkofft_hip.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")


@pytest.mark.skipif(not LIB.exists() or not (LLVM / "llvm-objdump").exists(), reason="needs the built library and ROCm's llvm-objdump")
def test_dht_table_kernel_has_no_fused_instruction():
    """-ffp-contract=off: every f64 and f32 operation of the restated sinf / cosf is one rounding (no v_fma* / v_fmac* / v_mad* of
    either width); the polynomials run in f64 and the table leaves in 16-byte stores."""
    sys.path.insert(0, str(ROOT / "tools"))
    from check_store_hazard import disassemble
    from test_trig_direct_cpu import _functions

    mine = {}
    for _, listing in disassemble(LIB):
        for func, lines in _functions(listing):
            if "dht_table_kernel" in func:
                mine[func] = lines
    assert len(mine) == 1, sorted(mine)
    bad = re.compile(r"^\s*(v_fma\w*|v_pk_fma\w*|v_fmac\w*|v_mac_\w*|v_mad_\w*|v_mfma\w*|v_dot\w*)\b")
    for func, lines in mine.items():
        hits = [ln for ln in lines if bad.match(ln)]
        assert not hits, f"{func}: {hits[:3]}"
        assert any(re.match(r"^\s*v_mul_f64", ln) for ln in lines) and any(re.match(r"^\s*v_add_f64", ln) for ln in lines), func
        assert any(re.match(r"^\s*v_cvt_f32_f64", ln) for ln in lines), func
        assert any("dwordx4" in ln and "store" in ln for ln in lines), func


def test_hartley_tables_under_asan_ubsan(tmp_path):
    """The host table, trig and window code in a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer."""
    exe = tmp_path / "sanitize_hartley_tables"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", "-ffp-contract=off"]
    subprocess.run(["g++", "-std=c++17", *flags, str(ROOT / "tests" / "cpp" / "sanitize_hartley_tables.cpp"),
                    str(ROOT / "kofft_amd" / "csrc" / "tables.cpp"), "-lm", "-pthread", "-o", str(exe)], check=True, capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert res.returncode == 0, res.stdout + res.stderr
    assert "0 problems" in res.stdout
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
