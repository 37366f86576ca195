"""Overlap-save convolution / correlation of rows without a GPU: the test oracle against numpy's float64 convolve and
correlate, pins of the definition, the default-block rule at its corners, and the argument checks of the C ABI and of the Python entry
points, which come before any device is touched."""
import ctypes as C

import numpy as np
import pytest

from conftest import seeded
from convolve_oracle import convolve_ref


def _rel_l2(got, want):
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def _bound(block):
    """The oracle's relative L2 error against float64 grows with the block through the reference's twiddle recurrence (as
    tests/test_hilbert_cpu.py notes for n): measured 3.9e-8 at block 2, 1.2e-6 at 32, 3.7e-5 at 1024, 3.2e-4 at 4096."""
    return 1e-6 + 2e-7 * block


def _f64(x, h, correlate):
    x64, h64 = x.astype(np.float64), h.astype(np.float64).reshape(-1, h.shape[-1])
    op = (lambda a, b: np.correlate(a, b, "full")) if correlate else np.convolve
    return np.stack([op(r, h64[i if h64.shape[0] > 1 else 0]) for i, r in enumerate(x64)])


# (block, nx, nh): measured relative L2 error of the oracle on uniform(-1, 1) data, convolve / correlate
SHAPES = [(2, 5, 2),         # 3.6e-8 / 4.0e-8
          (32, 20, 5),       # 7.2e-7 / 8.5e-7
          (32, 100, 32),     # 1.2e-6 / 1.1e-6   (block == nh: hop 1)
          (64, 1000, 17),    # 6.4e-7 / 5.8e-7
          (1024, 5000, 257),  # 3.7e-5 / 3.6e-5
          (4096, 20000, 1025),  # 2.4e-4 / 2.3e-4
          (4096, 9000, 4096)]  # 3.1e-4 / 3.1e-4  (block == nh at the largest fused block)


@pytest.mark.parametrize("correlate", [False, True])
@pytest.mark.parametrize("block,nx,nh", SHAPES)
def test_oracle_matches_float64(oracle, block, nx, nh, correlate):
    """The oracle's f32 result against numpy.convolve / numpy.correlate(.., "full") in float64; the bound leaves 2.5x over the
    measured value at block 4096 and more below (figures beside SHAPES)."""
    rng = seeded(9100 + block + nh)
    x = rng.uniform(-1, 1, (3, nx)).astype(np.float32)
    h = rng.uniform(-1, 1, nh).astype(np.float32)
    got = convolve_ref(x, h, block, correlate)
    assert got.dtype == np.float32 and got.shape == (3, nx + nh - 1)
    err = _rel_l2(got.astype(np.float64), _f64(x, h, correlate))
    print(f"block={block} nx={nx} nh={nh} correlate={correlate}: {err:.3g} (bound {_bound(block):.3g})")
    assert err <= _bound(block)


def test_oracle_per_row_filters(oracle):
    """One filter per row (measured 6.0e-7 at block 64, nx 300, nh 20): each row meets its own taps."""
    rng = seeded(9201)
    x = rng.uniform(-1, 1, (4, 300)).astype(np.float32)
    h = rng.uniform(-1, 1, (4, 20)).astype(np.float32)
    for correlate in (False, True):
        err = _rel_l2(convolve_ref(x, h, 64, correlate).astype(np.float64), _f64(x, h, correlate))
        print(f"per-row correlate={correlate}: {err:.3g}")
        assert err <= _bound(64)


@pytest.mark.parametrize("block", [2, 4])
def test_unit_impulse_returns_the_rows_bits_where_the_arithmetic_is_exact(oracle, block):
    """h = [1]: H is (1, 0) in every bin and the product is X.  At blocks 2 and 4 on small integers every butterfly and the 1 / block
    scale are exact, so the row comes back bit for bit.  (At larger blocks ifft(fft(x)) is not x in f32 -- measured 6.5e-7 relative
    at block 32 -- and the pin below holds to the bound instead.)"""
    x = seeded(9300 + block).integers(1, 9, (2, 3 * block + 1)).astype(np.float32)
    assert convolve_ref(x, np.ones(1, np.float32), block).tobytes() == x.tobytes()
    got = convolve_ref(x, np.array([1, 0], np.float32), block)  # the impulse with a zero tap behind it: one more output, a zero
    assert np.array_equal(got[:, :-1], x) and not got[:, -1].any()


@pytest.mark.parametrize("block", [2, 32, 256, 4096])
def test_single_tap_scales_the_row(oracle, block):
    """nh == 1 (hop == block, no overlap): the result is h[0] * x to the bound of test_oracle_matches_float64; the unit impulse is
    the case h[0] = 1 (measured 2.1e-8 at block 2, 6.5e-7 at 32, 6.2e-7 at 256, 6.6e-7 at 4096)."""
    x = seeded(9400 + block).uniform(-1, 1, (2, 2 * block + 3)).astype(np.float32)
    for tap in (1.0, -2.5):
        got = convolve_ref(x, np.array([tap], np.float32), block)
        assert got.shape == x.shape
        err = _rel_l2(got.astype(np.float64), x.astype(np.float64) * tap)
        print(f"block={block} tap={tap}: {err:.3g}")
        assert err <= _bound(block)


def test_one_block_per_row_equals_many_blocks(oracle):
    """The same convolution with one 1024-point block per row and with 64-point blocks: different bits, the same values to the sum
    of the two bounds (measured 3.1e-5)."""
    rng = seeded(9500)
    x = rng.uniform(-1, 1, (3, 900)).astype(np.float32)
    h = rng.uniform(-1, 1, 33).astype(np.float32)
    one, many = convolve_ref(x, h, 1024), convolve_ref(x, h, 64)
    err = _rel_l2(many.astype(np.float64), one.astype(np.float64))
    print(f"one against many: {err:.3g}")
    assert err <= _bound(1024) + _bound(64)


def _block(hiplib, nx, nh):
    out = C.c_size_t(0)
    assert hiplib.kofft_hip_convolve_block(C.c_size_t(nx), C.c_size_t(nh), C.byref(out)) == 0
    return out.value


def test_default_block_rule(hiplib):
    """kofft_hip_convolve_block: p = next_pow2(nx + nh - 1); p if p <= 4096, else 2048 if nh <= 1024 (the measured
    choice on long rows), else 4096 if nh <= 2048, else min(p, next_pow2(2 nh))."""
    assert _block(hiplib, 1, 1) == 1
    assert _block(hiplib, 5, 2) == 8          # full 6
    assert _block(hiplib, 200, 57) == 256     # full 256 exactly
    assert _block(hiplib, 201, 57) == 512
    assert _block(hiplib, 3000, 1097) == 4096  # p == 4096: one block per row
    assert _block(hiplib, 4000, 97) == 4096   # full 4096 exactly: p == 4096, still one block per row
    assert _block(hiplib, 4001, 97) == 2048   # p == 8192, a short filter
    assert _block(hiplib, 7169, 1024) == 2048  # p == 8192, nh == 1024: the last filter 2048 takes
    assert _block(hiplib, 7168, 1025) == 4096  # p == 8192, nh == 1025
    assert _block(hiplib, 6145, 2048) == 4096  # p == 8192, nh == 2048: the last filter 4096 takes
    assert _block(hiplib, 6144, 2049) == 8192  # p == 8192, nh == 2049: min(8192, 8192)
    assert _block(hiplib, 1 << 24, 64) == 2048
    assert _block(hiplib, 1 << 24, 1024) == 2048
    assert _block(hiplib, 1 << 24, 1025) == 4096
    assert _block(hiplib, 1 << 24, 2049) == 8192
    assert _block(hiplib, 1 << 24, 4097) == 16384
    assert _block(hiplib, 10, 5000) == 8192   # nh > nx: p == 8192 < next_pow2(2 nh) == 16384
    assert _block(hiplib, 3, 100) == 128      # nh > nx below 4096
    assert _block(hiplib, 40000, 40000) == 131072  # (beyond the transform's range: the call itself reports UNSUPPORTED)
    null = C.POINTER(C.c_size_t)()
    out = C.c_size_t(7)
    assert hiplib.kofft_hip_convolve_block(C.c_size_t(0), C.c_size_t(4), C.byref(out)) == 1
    assert hiplib.kofft_hip_convolve_block(C.c_size_t(4), C.c_size_t(0), C.byref(out)) == 1
    assert out.value == 7
    assert hiplib.kofft_hip_convolve_block(C.c_size_t(4), C.c_size_t(4), null) == -3


def test_python_default_block_is_the_librarys(hiplib):
    from kofft_amd import convolve

    for nx, nh in [(5, 2), (3000, 1097), (6144, 2049), (10, 5000)]:
        assert convolve.default_block(nx, nh) == _block(hiplib, nx, nh)


@pytest.mark.parametrize("entry", ["kofft_hip_convolve_f32", "kofft_hip_dev_convolve_f32"])
def test_abi_argument_order_null_context(hiplib, entry):
    """rows == 0 or out_len == 0 -> Ok; nx == 0 or nh == 0 -> EmptyInput; block not a power of two -> NonPowerOfTwoNoStd; block < nh,
    filters not 1 or rows, a window past the full result -> MismatchedLengths; an unknown flag -> InvalidValue; block > 65536 ->
    UNSUPPORTED; then the null context: each check before the next, none of them touching a device."""
    fn = getattr(hiplib, entry)
    null = C.c_void_p(None)
    buf = np.zeros(64, np.float32)
    p = C.c_void_p(buf.ctypes.data)
    sz = C.c_size_t

    def call(rows=2, nx=20, nh=5, filters=1, block=8, flags=0, first=0, count=24, ctx=null, x=p, h=p, out=p):
        return fn(ctx, x, sz(rows), sz(nx), h, sz(filters), sz(nh), sz(block), C.c_uint(flags), out, sz(first), sz(count))

    assert call() == -3                       # a valid request, null context
    assert call(rows=0, nx=0, block=3) == 0   # rows first
    assert call(count=0, nh=0, block=3) == 0  # out_len with it
    assert call(nx=0, block=3) == 1
    assert call(nh=0, block=3) == 1
    assert call(block=12, nh=20) == 2         # not a power of two, before block < nh
    assert call(block=4) == 3                 # block < nh
    assert call(block=4, filters=3, flags=2) == 3
    assert call(filters=3, first=30) == 3     # filters not in {1, rows}
    assert call(filters=2) == -3              # filters == rows
    assert call(first=1, count=24, flags=2) == 3  # window past the full result, before the flags
    assert call(first=24, count=1) == 3
    assert call(first=23, count=1) == -3
    assert call(flags=2, block=1 << 17) == 6  # an unknown flag, before the block's range
    assert call(flags=3) == 6
    assert call(flags=1) == -3                # correlate
    assert call(block=1 << 17) == -2
    assert call(block=1 << 16) == -3          # the largest block is a valid request
    assert call(block=0) == -3                # the default block (32 here)
    assert call(block=0, nh=40000, nx=40000, count=1) == -2  # whose default lies beyond the range
    assert call(x=None) == -3 and call(h=None) == -3 and call(out=None) == -3
    assert hiplib.kofft_hip_set_convolve_fused(null, 0) == -3
    assert hiplib.kofft_hip_set_convolve_fused(null, 1) == -3


def test_python_errors_need_no_device(monkeypatch):
    """convolve / correlate raise their shape, mode and block errors before any context is created."""
    import kofft_amd
    from kofft_amd import api, convolve

    def no_device(*a, **k):
        raise AssertionError("a context was created")

    monkeypatch.setattr(api, "HipFftImpl", no_device)
    monkeypatch.setattr(convolve, "_default", None)
    E = kofft_amd.FftError
    x = np.ones((2, 10), np.float32)
    for fn in (kofft_amd.convolve.convolve, kofft_amd.convolve.correlate):
        for args, code in [(([], [1.0]), E.EmptyInput), ((x, []), E.EmptyInput), ((np.ones((2, 0), np.float32), [1.0]), E.EmptyInput),
                           ((x, np.ones((3, 4), np.float32)), E.MismatchedLengths)]:
            with pytest.raises(E) as e:
                fn(*args)
            assert e.value == E(code)
        with pytest.raises(E) as e:
            fn(x, np.ones(4, np.float32), block=12)
        assert e.value == E(E.NonPowerOfTwoNoStd)
        with pytest.raises(E) as e:
            fn(x, np.ones(5, np.float32), block=4)
        assert e.value == E(E.MismatchedLengths)
        with pytest.raises(E) as e:
            fn(x, np.ones(11, np.float32), mode="valid")
        assert e.value == E(E.MismatchedLengths)
        with pytest.raises(ValueError):
            fn(x, np.ones(3, np.float32), mode="wrap")
        with pytest.raises(TypeError):
            fn(np.ones((2, 2, 4), np.float32), np.ones(3, np.float32))
    # with a valid request the context is what is asked for next
    with pytest.raises(AssertionError, match="a context was created"):
        kofft_amd.convolve.convolve(x, np.ones(3, np.float32))
