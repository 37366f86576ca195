"""Filter-bank convolution of rows and the Morlet scalogram on it without a GPU: the bank oracle against the
one-filter oracle bit for bit and against numpy's float64 convolve / correlate, the Morlet taps, the scalogram of a pure tone computed
by the oracle, and the argument checks of the C ABI and of the Python entry points, which come before any device is touched."""
import ctypes as C

import numpy as np
import pytest

from conftest import seeded
from convolve_bank_oracle import convolve_bank_ref
from convolve_oracle import convolve_ref

F = np.float32


def _rel_l2(got, want):
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def _bound(block):
    """convolve's bound (tests/test_convolve_cpu.py): the oracle's error grows with the block through the twiddle recurrence."""
    return 1e-6 + 2e-7 * block


def _ctaps(rng, filters, nh):
    return (rng.uniform(-1, 1, (filters, nh)) + 1j * rng.uniform(-1, 1, (filters, nh))).astype(np.complex64)


@pytest.mark.parametrize("correlate", [False, True])
@pytest.mark.parametrize("block,nx,nh", [(2, 5, 2), (32, 100, 9), (32, 40, 32), (256, 700, 65), (1024, 2500, 257), (4096, 9000, 1025)])
def test_real_taps_real_part_is_the_one_filter_oracle(oracle, block, nx, nh, correlate):
    """With real taps and the real part kept, (row, filter) is convolve_ref(x[row], h[filter], block) bit for bit."""
    rng = seeded(11000 + block + nh)
    x = rng.uniform(-1, 1, (3, nx)).astype(F)
    h = rng.uniform(-1, 1, (4, nh)).astype(F)
    got = convolve_bank_ref(x, h, block, correlate)
    assert got.dtype == F and got.shape == (3, 4, nx + nh - 1)
    for f in range(4):
        assert got[:, f].tobytes() == convolve_ref(x, h[f], block, correlate).tobytes(), f"filter {f}"


@pytest.mark.parametrize("correlate", [False, True])
@pytest.mark.parametrize("block,nx,nh", [(32, 100, 9), (256, 700, 65), (1024, 2500, 257), (4096, 9000, 1025)])
def test_complex_taps_match_float64(oracle, block, nx, nh, correlate):
    """Complex taps against numpy.convolve / numpy.correlate(.., "full") in float64 (numpy.correlate conjugates its second argument):
    the complex values and the magnitudes stay inside convolve's bound (measured at most 8.9e-7, 9.9e-7, 3.8e-5 and 2.4e-4 at the
    four blocks); the real part is the complex value's."""
    rng = seeded(11100 + block + nh)
    x = rng.uniform(-1, 1, (2, nx)).astype(F)
    h = _ctaps(rng, 3, nh)
    op = (lambda a, b: np.correlate(a, b, "full")) if correlate else np.convolve
    want = np.stack([[op(r.astype(np.float64), t.astype(np.complex128)) for t in h] for r in x])
    got = convolve_bank_ref(x, h, block, correlate, "complex")
    mag = convolve_bank_ref(x, h, block, correlate, "magnitude")
    assert got.dtype == np.complex64 and mag.dtype == F and got.shape == mag.shape == (2, 3, nx + nh - 1)
    err_c, err_m = _rel_l2(got.astype(np.complex128), want), _rel_l2(mag.astype(np.float64), np.abs(want))
    print(f"block={block} nx={nx} nh={nh} correlate={correlate}: complex {err_c:.3g} magnitude {err_m:.3g} (bound {_bound(block):.3g})")
    assert err_c <= _bound(block) and err_m <= _bound(block)
    assert convolve_bank_ref(x, h, block, correlate, "real").tobytes() == np.ascontiguousarray(got.real).tobytes()
    re, im = np.ascontiguousarray(got.real), np.ascontiguousarray(got.imag)
    assert mag.tobytes() == np.sqrt(re * re + im * im).tobytes()


def test_correlate_conjugates_and_reverses(oracle):
    """correlate with complex taps is convolve with conj(h[::-1]), bit for bit: numpy.correlate's definition."""
    rng = seeded(11200)
    x = rng.uniform(-1, 1, (2, 300)).astype(F)
    h = _ctaps(rng, 3, 20)
    a = convolve_bank_ref(x, h, 64, True, "complex")
    b = convolve_bank_ref(x, np.conj(h[:, ::-1]), 64, False, "complex")
    assert a.tobytes() == b.tobytes()


def test_morlet_taps():
    """Shapes, the amplitude at the centre, truncation at ceil(support s) and Hermitian symmetry."""
    from kofft_amd import wavelet

    assert "morlet_taps" in wavelet.__all__ and "cwt" in wavelet.__all__
    scales = [2.0, 3.5, 10.0]
    taps = wavelet.morlet_taps(scales)
    assert taps.dtype == np.complex64 and taps.shape == (3, 81)  # 2 ceil(4 * 10) + 1
    assert wavelet.morlet_taps([1.3], w0=5.0, support=3.0).shape == (1, 9)  # 2 ceil(3.9) + 1
    mid = 40
    for k, s in enumerate(scales):
        assert taps[k, mid] == np.complex64(np.pi ** -0.25 / np.sqrt(s))
        half = int(np.ceil(4.0 * s))
        assert not taps[k, :mid - half].any() and not taps[k, mid + half + 1:].any()
        assert taps[k, mid - half] != 0 and taps[k, mid + half] != 0
        assert np.array_equal(taps[k], np.conj(taps[k, ::-1]))  # psi(-t) = conj(psi(t)), exactly: cos is even, sin odd
        t = (np.arange(81) - mid) / s
        want = np.pi ** -0.25 * np.exp(1j * 6.0 * t - 0.5 * t * t) / np.sqrt(s)
        want[np.abs(np.arange(81) - mid) > half] = 0
        assert np.allclose(taps[k], want, rtol=1e-6, atol=1e-9)
    for bad in ([], [0.0], [-1.0], [np.inf], [[1.0, 2.0]]):
        with pytest.raises(ValueError):
            wavelet.morlet_taps(bad)
    with pytest.raises(ValueError):
        wavelet.morlet_taps([1.0], support=0.0)


def test_scalogram_of_a_tone_peaks_at_its_scale(oracle):
    """A pure tone of f0 cycles per sample through the oracle's "same" correlation with a geometric ladder of Morlet scales: away
    from the ends the magnitude is largest at the ladder's scale nearest w0 / (2 pi f0) (on a log axis), at every sample."""
    from kofft_amd import wavelet

    w0, f0, nx = 6.0, 0.05, 1200
    scales = 4.0 * 2.0 ** (np.arange(10) / 3.0)  # 4 .. 32
    want_k = int(np.argmin(np.abs(np.log(scales) - np.log(w0 / (2 * np.pi * f0)))))
    assert 0 < want_k < 9
    x = np.cos(2 * np.pi * f0 * np.arange(nx) + 0.3).astype(F)[None, :]
    taps = wavelet.morlet_taps(scales, w0)
    nh = taps.shape[1]
    mag = convolve_bank_ref(x, taps, 1024, True, "magnitude")[0, :, (nh - 1) // 2:(nh - 1) // 2 + nx]
    assert mag.shape == (10, nx)
    inner = mag[:, nh:-nh]
    assert (np.argmax(inner, axis=0) == want_k).all()


@pytest.mark.parametrize("entry", ["kofft_hip_convolve_bank_f32", "kofft_hip_dev_convolve_bank_f32"])
def test_abi_argument_order_null_context(hiplib, entry):
    """rows == 0, filters == 0 or out_len == 0 -> Ok; nx == 0 or nh == 0 -> EmptyInput; block not a power of two ->
    NonPowerOfTwoNoStd; block < nh, a window past the full result -> MismatchedLengths; a flag bit above bit 3 or output kind 3 ->
    InvalidValue; block > 65536 -> UNSUPPORTED; then the null pointers and the null context: each check before the next, none of
    them touching a device."""
    fn = getattr(hiplib, entry)
    null = C.c_void_p(None)
    buf = np.zeros(64, F)
    p = C.c_void_p(buf.ctypes.data)
    sz = C.c_size_t

    def call(rows=2, nx=20, nh=5, filters=3, block=8, flags=0, first=0, count=24, ctx=null, x=p, h=p, out=p):
        return fn(ctx, x, sz(rows), sz(nx), h, sz(filters), sz(nh), sz(block), C.c_uint(flags), out, sz(first), sz(count))

    assert call() == -3                       # a valid request, null context
    assert call(rows=0, nx=0, block=3) == 0   # rows first
    assert call(filters=0, nh=0, block=3) == 0
    assert call(count=0, nh=0, block=3) == 0
    assert call(nx=0, block=3) == 1
    assert call(nh=0, block=3) == 1
    assert call(block=12, nh=20) == 2         # not a power of two, before block < nh
    assert call(block=4) == 3                 # block < nh
    assert call(block=4, flags=16) == 3
    assert call(first=1, count=24, flags=16) == 3  # window past the full result, before the flags
    assert call(first=24, count=1) == 3
    assert call(first=23, count=1) == -3
    assert call(flags=16, block=1 << 17) == 6  # a flag bit above bit 3, before the block's range
    assert call(flags=12, block=1 << 17) == 6  # output kind 3
    assert call(flags=1 << 31) == 6
    for flags in (1, 2, 3, 4, 8, 7, 11):       # correlate, complex taps, the three kinds
        assert call(flags=flags) == -3
    assert call(block=1 << 17) == -2
    assert call(block=1 << 16) == -3          # the largest block is a valid request
    assert call(block=0) == -3                # the default block (32 here)
    assert call(block=0, nh=40000, nx=40000, count=1) == -2  # whose default lies beyond the range
    assert call(filters=100) == -3            # any number of filters
    assert call(x=None) == -3 and call(h=None) == -3 and call(out=None) == -3
    assert hiplib.kofft_hip_set_convolve_bank_fused(null, 0) == -3
    assert hiplib.kofft_hip_set_convolve_bank_fused(null, 1) == -3


def test_python_errors_need_no_device(monkeypatch):
    """convolve_bank / correlate_bank / cwt raise their shape, mode, kind and block errors before any context is created."""
    import kofft_amd
    from kofft_amd import api, convolve, wavelet

    def no_device(*a, **k):
        raise AssertionError("a context was created")

    monkeypatch.setattr(api, "HipFftImpl", no_device)
    monkeypatch.setattr(convolve, "_default", None)
    E = kofft_amd.FftError
    x = np.ones((2, 10), F)
    bank = np.ones((3, 4), F)
    for fn in (convolve.convolve_bank, convolve.correlate_bank):
        for args, code in [(([], bank), E.EmptyInput), ((x, np.ones((3, 0), F)), E.EmptyInput), ((np.ones((2, 0), F), bank), E.EmptyInput)]:
            with pytest.raises(E) as e:
                fn(*args)
            assert e.value == E(code)
        with pytest.raises(E) as e:
            fn(x, bank, block=12)
        assert e.value == E(E.NonPowerOfTwoNoStd)
        with pytest.raises(E) as e:
            fn(x, np.ones((3, 5), F), block=4)
        assert e.value == E(E.MismatchedLengths)
        with pytest.raises(E) as e:
            fn(x, np.ones((3, 11), np.complex64), mode="valid")
        assert e.value == E(E.MismatchedLengths)
        with pytest.raises(ValueError):
            fn(x, bank, mode="wrap")
        with pytest.raises(ValueError):
            fn(x, bank, out="power")
        with pytest.raises(TypeError):
            fn(x, np.ones(4, F))  # a bank is 2-D
        with pytest.raises(TypeError):
            fn(np.ones((2, 2, 4), F), bank)
    with pytest.raises(ValueError):
        wavelet.cwt(x)  # neither scales nor taps
    with pytest.raises(ValueError):
        wavelet.cwt(x, [2.0], taps=bank)
    with pytest.raises(ValueError):
        wavelet.cwt(x, [2.0], out="power")
    with pytest.raises(E) as e:
        wavelet.cwt(x, [2.0], block=4)  # 17 taps
    assert e.value == E(E.MismatchedLengths)
    # with a valid request the context is what is asked for next
    with pytest.raises(AssertionError, match="a context was created"):
        convolve.convolve_bank(x, bank)
    with pytest.raises(AssertionError, match="a context was created"):
        wavelet.cwt(x, [1.0, 2.0])
