"""The wavelet transforms on the host side (no GPU): the coefficients' bits, the test oracle against a scalar line-by-line transcription
of wavelet.rs, the reference's own assertions, the MismatchedLengths rule of the multi-level inverse, the argument checks of the C ABI
and of kofft_amd.wavelet, and the machine code of the new kernels (nothing fused, no MFMA)."""
import ctypes as C
import re
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

import wavelet_oracle as wo
from rowcheck import assert_rows_equal

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
LIB = ROOT / "kofft_amd" / "lib" / "libkofft_hip.so"
LLVM = Path("/opt/rocm/lib/llvm/bin")


def _f32_nearest(dec: str) -> np.float32:
    """The f32 nearest to the decimal string (ties to even), by exact rational arithmetic."""
    q = Fraction(dec)
    c = np.float32(float(q))
    best = None
    for cand in (np.nextafter(c, F(-np.inf)), c, np.nextafter(c, F(np.inf))):
        err = abs(Fraction(float(cand)) - q)
        even = (int(np.array(cand).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, cand)
    return best[1]


@pytest.mark.parametrize("name", wo.NAMES[1:])
@pytest.mark.parametrize("inverse", [False, True])
def test_coefficients_are_the_nearest_f32(hiplib, name, inverse):
    """Every tap, in the oracle and in the library (kofft_hip_wavelet_taps_f32), is the correctly rounded f32 of wavelet.rs's string."""
    decs = wo.DECIMALS[(name, inverse)]
    want = [np.array([_f32_nearest(v) for v in half], F) for half in decs]
    lo, hi = wo.taps(name, inverse)
    assert lo.tobytes() == want[0].tobytes() and hi.tobytes() == want[1].tobytes()
    blo, bhi = (C.c_float * 8)(), (C.c_float * 8)()
    assert hiplib.kofft_hip_wavelet_taps_f32(wo.NAMES.index(name), int(inverse), blo, bhi) == 0
    L = wo.ntaps(name)
    got_lo, got_hi = np.array(blo[:], F), np.array(bhi[:], F)
    assert got_lo[:L].tobytes() == want[0].tobytes() and got_hi[:L].tobytes() == want[1].tobytes()
    assert not got_lo[L:].any() and not got_hi[L:].any()


# ---- a scalar transcription of wavelet.rs, line by line ----------------------------------------------------------------------------
def _reflect(idx, n):
    while idx < 0 or idx >= n:
        if idx < 0:
            idx = -idx
        else:
            idx = 2 * (n - 1) - idx
    return idx


def s_forward(name, x):
    n = len(x) // 2
    approx, detail = [F(0.0)] * n, [F(0.0)] * n
    length = len(x)
    if name == "haar":
        for i in range(n):
            approx[i] = (x[2 * i] + x[2 * i + 1]) / F(2.0)
            detail[i] = (x[2 * i] - x[2 * i + 1]) / F(2.0)
        return approx, detail
    h, g = wo.taps(name, False)
    for i in range(n):
        j = 2 * i
        if name == "db2":
            r = [x[_reflect(j + k, length)] for k in range(4)]
            approx[i] = h[0] * r[0] + h[1] * r[1] + h[2] * r[2] + h[3] * r[3]
            detail[i] = g[0] * r[0] + g[1] * r[1] + g[2] * r[2] + g[3] * r[3]
        else:
            for k in range(len(h)):
                val = x[_reflect(j + k, length)]
                approx[i] += h[k] * val
                detail[i] += g[k] * val
    return approx, detail


def s_inverse(name, a, d):
    n = len(a)
    length = n * 2
    output = [F(0.0)] * length
    if name == "haar":
        for i in range(n):
            output[2 * i] = a[i] + d[i]
            output[2 * i + 1] = a[i] - d[i]
        return output
    g, h = wo.taps(name, True)
    for i in range(n):
        j = 2 * i
        for k in range(len(g)):
            idx = _reflect(j + k, length)
            output[idx] += g[k] * a[i] + h[k] * d[i]
    return output


def s_forward_multi(name, x, levels):
    current = list(x)
    details = []
    for _ in range(levels):
        if len(current) % 2 != 0 and current:
            current.append(current[-1])
        avg, diff = s_forward(name, current)
        details.append(diff)
        current = avg
    return current, details


def s_inverse_multi(name, a, details):
    current = list(a)
    for d in reversed(details):
        if len(d) < len(current):
            raise wo.MismatchedLengths()  # the reference's out-of-bounds panic
        current = s_inverse(name, current, d)
    return current


_SPECIALS = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1.2e-38, np.inf, -np.inf, np.nan, 3e38, -3e38], F)


def _rows(n, seed):
    rng = np.random.default_rng(seed)
    rows = [rng.uniform(-1, 1, n).astype(F) for _ in range(2)]
    rows += [np.full(n, v, F) for v in (-0.0, 0.0, 1e-40, 3e38)]
    r = rng.uniform(-1, 1, n).astype(F)
    if n:
        r[rng.integers(0, n, max(1, n // 4))] = _SPECIALS[rng.integers(0, len(_SPECIALS), max(1, n // 4))]
    rows.append(r)
    rows.append(_SPECIALS[rng.integers(0, len(_SPECIALS), n)])
    return np.stack(rows).reshape(len(rows), n)


def _as(rows, n):
    return np.array(rows, F).reshape(len(rows), n)


LENGTHS = list(range(0, 41)) + [64, 99, 257]


@pytest.mark.parametrize("name", wo.NAMES)
def test_oracle_is_the_scalar_transcription(name):
    """Single level, both directions, lengths 0 .. 40 and a few larger, rows of +-0, subnormals, +-Inf and NaN."""
    with np.errstate(all="ignore"):
        for n in LENGTHS:
            x = _rows(n, 100 + n)
            a, d = wo.forward(name, x)
            sa = [s_forward(name, list(r)) for r in x]
            assert_rows_equal(a, _as([s[0] for s in sa], n // 2), f"{name} forward n={n}", nan_safe=True)
            assert_rows_equal(d, _as([s[1] for s in sa], n // 2), f"{name} forward detail n={n}", nan_safe=True)
            if n % 2 == 0:
                h = n // 2
                y = wo.inverse(name, x[:, :h], x[:, h:])
                sy = [s_inverse(name, list(r[:h]), list(r[h:])) for r in x]
                assert_rows_equal(y, _as(sy, n), f"{name} inverse n={n}", nan_safe=True)


@pytest.mark.parametrize("name", wo.NAMES)
def test_multi_level_oracle_is_the_scalar_transcription(name):
    """Multi level, lengths 0 .. 40 and a few larger, levels 0 .. 8: the padding, the detail lengths, the inverse's fold."""
    with np.errstate(all="ignore"):
        for n in LENGTHS:
            x = _rows(n, 200 + n)[:4]
            for levels in range(0, 9):
                a, ds = wo.forward_multi(name, x, levels)
                ref = [s_forward_multi(name, list(r), levels) for r in x]
                assert [dd.shape[1] for dd in ds] == wo.multi_lengths(n, levels)[1:]
                assert_rows_equal(a, _as([r[0] for r in ref], a.shape[1]), f"{name} n={n} L={levels}", nan_safe=True)
                for l, dd in enumerate(ds):
                    assert_rows_equal(dd, _as([r[1][l] for r in ref], dd.shape[1]), f"{name} n={n} L={levels} d{l}", nan_safe=True)
                try:
                    want = [s_inverse_multi(name, r[0], r[1]) for r in ref]
                except wo.MismatchedLengths:
                    with pytest.raises(wo.MismatchedLengths):
                        wo.inverse_multi(name, a, ds)
                    continue
                y = wo.inverse_multi(name, a, ds)
                assert_rows_equal(y, _as(want, y.shape[1]), f"{name} inverse n={n} L={levels}", nan_safe=True)


def test_reference_assertions_on_the_oracle():
    """wavelet.rs's own tests (569-732), on the oracle."""
    x = np.array([[1, 2, 3, 4]], F)
    assert np.all(np.abs(wo.inverse("haar", *wo.forward("haar", x)) - x) < 1e-5)
    xs = np.array([[1, 2, 3, 4, 5, 6, 7, 8], [5, 6, 7, 8, 1, 2, 3, 4]], F)
    assert np.all(np.abs(wo.inverse("haar", *wo.forward("haar", xs)) - xs) < 1e-6)
    rec = wo.inverse("db2", *wo.forward("db2", xs))
    assert np.max(np.abs(xs - rec)) < np.max(np.abs(xs))
    a, d = wo.forward_multi("haar", xs[:1], 3)
    assert np.all(np.abs(wo.inverse_multi("haar", a, d) - xs[:1]) < 1e-5)
    a, d = wo.forward_multi("haar", np.array([[1, 2, 3, 4], [5, 6, 7, 8]], F), 2)
    assert np.all(np.abs(wo.inverse_multi("haar", a, d) - np.array([[1, 2, 3, 4], [5, 6, 7, 8]], F)) < 1e-5)
    for name in ("sym4", "coif1"):
        a, d = wo.forward_multi(name, xs[:1], 2)
        assert wo.inverse_multi(name, a, d).shape[1] == 8


def test_mismatched_lengths_exactly_when_an_inner_length_is_odd(hiplib):
    """The multi-level inverse of the forward's own output panics in the reference exactly when one of a_1 .. a_{L-1} is odd: the
    oracle raises then and only then, and the C ABI returns MISMATCHED_LENGTHS (3) then and only then, before the null context."""
    for n in range(1, 41):
        for levels in range(0, 7):
            lens = wo.multi_lengths(n, levels)
            odd = any(m % 2 for m in lens[1:levels])
            x = np.arange(n, dtype=F).reshape(1, n)
            a, ds = wo.forward_multi("db4", x, levels)
            if odd:
                with pytest.raises(wo.MismatchedLengths):
                    wo.inverse_multi("db4", a, ds)
            else:
                assert wo.inverse_multi("db4", a, ds).shape[1] == lens[levels] << levels
            dl = (C.c_size_t * max(1, levels))(*lens[1:])
            rc = hiplib.kofft_hip_idwt_multi_f32(None, 2, None, None, dl, None, lens[levels], 1, levels)
            assert rc == (3 if odd else -3), (n, levels, rc)


def test_argument_checks_in_order_with_a_null_context(hiplib):
    """include/kofft_hip.h: the wavelet id, batch / length zero, MISMATCHED_LENGTHS, UNSUPPORTED, then null pointers."""
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    one = (C.c_size_t * 2)(4, 8)
    for fn in (hiplib.kofft_hip_dwt_f32, hiplib.kofft_hip_dwt_f32_dev, hiplib.kofft_hip_idwt_f32, hiplib.kofft_hip_idwt_f32_dev):
        assert fn(None, 5, p, p, p, 4, 1) == 6 and fn(None, -1, None, None, None, 0, 0) == 6
        assert fn(None, 0, None, None, None, 4, 0) == 0 and fn(None, 2, None, None, None, 0, 3) == 0
        assert fn(None, 1, None, None, None, 1 << 27, 1) == -2
        assert fn(None, 1, p, p, p, 8, 1) == -3
    assert hiplib.kofft_hip_idwt_f32(None, 1, None, None, None, (1 << 25) + 1, 1) == -2  # the output row is 2n
    assert hiplib.kofft_hip_dwt_f32(None, 1, None, None, None, 1 << 26, 1) == -3
    for fn in (hiplib.kofft_hip_dwt_multi_f32, hiplib.kofft_hip_dwt_multi_f32_dev):
        assert fn(None, 7, p, p, p, 4, 1, 2) == 6
        assert fn(None, 3, None, None, None, 0, 1, 2) == 0 and fn(None, 3, None, None, None, 4, 0, 2) == 0
        assert fn(None, 3, None, None, None, (1 << 26) + 1, 1, 2) == -2 and fn(None, 3, None, None, None, 4, 1, 65) == -2
        assert fn(None, 3, p, p, p, 4, 1, 64) == -3 and fn(None, 3, p, p, None, 4, 1, 0) == -3
    for fn in (hiplib.kofft_hip_idwt_multi_f32, hiplib.kofft_hip_idwt_multi_f32_dev):
        assert fn(None, 9, p, p, one, p, 2, 1, 2) == 6
        assert fn(None, 4, None, None, None, None, 0, 1, 2) == 0 and fn(None, 4, None, None, None, None, 2, 0, 2) == 0
        assert fn(None, 4, p, p, one, p, 5, 1, 2) == 3  # (8 >= 5 first, then 4 < 10)
        assert fn(None, 4, p, p, None, p, 2, 1, 2) == -3  # the lengths cannot be read
        big = (C.c_size_t * 65)(*([1 << 40] * 65))
        assert fn(None, 4, p, p, big, p, 2, 1, 65) == -2 and fn(None, 4, p, p, one, p, 1 << 25, 1, 2) == 3
        # levels > 64 before any length is read: a huge count with a two-entry array, and 65 lengths that would mismatch
        assert fn(None, 4, p, p, one, p, 2, 1, (1 << 64) - 1) == -2 and fn(None, 4, p, p, (C.c_size_t * 65)(*([1] * 65)), p, 2, 1, 65) == -2
        assert fn(None, 4, p, p, (C.c_size_t * 2)(1 << 26, 1 << 25), p, 1 << 25, 1, 2) == -2  # the output row is 2^27
        assert fn(None, 4, p, p, one, p, 2, 1, 2) == -3 and fn(None, 4, p, None, one, p, 2, 1, 0) == -3
    lens = (C.c_size_t * 5)()
    assert hiplib.kofft_hip_dwt_multi_lengths(9, 65, lens) == -2 and hiplib.kofft_hip_dwt_multi_lengths(9, 4, None) == -3
    assert hiplib.kofft_hip_dwt_multi_lengths(9, 4, lens) == 0 and list(lens) == [9, 5, 3, 2, 1]
    assert hiplib.kofft_hip_wavelet_taps_f32(5, 0, p, p) == 6 and hiplib.kofft_hip_wavelet_taps_f32(1, 0, None, p) == -3
    assert hiplib.kofft_hip_set_wavelet_fused(None, 1) == -3


def test_python_errors_before_any_device():
    import kofft_amd
    from kofft_amd import wavelet as wv

    with pytest.raises(kofft_amd.FftError) as e:
        wv.db4_inverse(np.zeros(4, F), np.zeros(3, F))
    assert e.value == kofft_amd.FftError(kofft_amd.FftError.MismatchedLengths)
    with pytest.raises(kofft_amd.FftError):
        wv.sym4_inverse_multi(np.zeros(2, F), [np.zeros(3, F), np.zeros(3, F)])  # 3 >= 2, then 3 < 4
    with pytest.raises(kofft_amd.FftError):
        wv.multi_level_inverse_batch([np.zeros(2, F), np.zeros(2, F)], [[np.zeros(4, F)], [np.zeros(1, F)]], wv.haar_inverse)
    with pytest.raises(kofft_amd.DeviceError):
        wv.haar_forward_multi(np.zeros(4, F), 65)
    with pytest.raises(kofft_amd.DeviceError):
        wv.batch_forward([np.zeros(4, F), np.zeros((1 << 26) + 2, F)])
    with pytest.raises(ValueError):
        wv.multi_level_forward(np.zeros(4, F), -1, wv.db2_forward)
    with pytest.raises(TypeError):
        wv.coif1_forward(np.zeros((2, 4), F))
    with pytest.raises(kofft_amd.FftError):
        kofft_amd.api.wavelet_id("db8")
    a, d = wv.db2_forward(np.zeros(1, F))
    assert a.shape == (0,) and d.shape == (0,)
    assert wv.haar_inverse(np.zeros(0, F), np.zeros(0, F)).shape == (0,)
    a, ds = wv.db4_forward_multi(np.zeros(0, F), 3)
    assert a.shape == (0,) and [x.shape for x in ds] == [(0,)] * 3
    # a foreign callable: the reference's loop in Python, padding included
    seen = []

    def fwd(x):
        seen.append(len(x))
        return x[0::2].copy(), x[1::2].copy()

    a, ds = wv.multi_level_forward(np.arange(5, dtype=F), 3, fwd)
    assert seen == [6, 4, 2] and a.tolist() == [0.0] and [x.tolist() for x in ds] == [[1, 3, 4], [2, 4], [4]]
    assert wv._default is None, "a context was created before the errors"


def _functions(listing):
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


@pytest.mark.skipif(not LIB.exists() or not (LLVM / "llvm-objdump").exists(), reason="needs the built library and ROCm's llvm-objdump")
def test_wavelet_kernels_have_no_fused_or_mfma_instruction():
    """-ffp-contract=off and the kernels' own arithmetic: one multiply and one add per term (wavelet.rs does not fuse)."""
    sys.path.insert(0, str(ROOT / "tools"))
    from check_store_hazard import disassemble

    funcs = {}
    for _, listing in disassemble(LIB):
        for func, lines in _functions(listing):
            if "wavelet_" in func and "_kernel" in func:
                funcs[func] = lines
    assert len(funcs) == 20, sorted(funcs)
    bad = re.compile(r"^\s*(v_fma\w*|v_pk_fma\w*|v_fmac\w*|v_mac_\w*|v_mad_f32|v_mad_legacy\w*|v_mad_mix\w*|v_mfma\w*|v_dot\w*)\b")
    for func, lines in funcs.items():
        hits = [ln for ln in lines if bad.match(ln)]
        assert not hits, f"{func}: {hits[:3]}"
        assert not any("scratch_" in ln for ln in lines), f"{func} spills to scratch"
