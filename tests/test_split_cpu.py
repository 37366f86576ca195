"""FftImpl::fft_split / ifft_split (fft.rs:1365-1439) without a GPU: the C ABI's argument checks, which come before any device is
touched, the Python mirrors' length checks, the SplitComplex / ComplexVec types, and the test oracle (tests/split_oracle.py) against the
second restatement of fft_split_simd's stages (tests/ref_restatement.py)."""
import ctypes as C

import numpy as np
import pytest

import ref_restatement as rr
from conftest import bits_equal, seeded
from split_oracle import split_ref

HOST = ["kofft_hip_fft_split_c32", "kofft_hip_fft_split_c64"]
DEV = ["kofft_hip_dev_fft_split_c32", "kofft_hip_dev_fft_split_c64"]


@pytest.mark.parametrize("entry", HOST + DEV)
@pytest.mark.parametrize("inverse", [0, 1])
def test_abi_argument_order_null_context(hiplib, entry, inverse):
    """batch == 0 -> Ok, n == 0 -> EmptyInput, n beyond the complex transform's range (2^26 for powers of two, 2^25 otherwise) ->
    UNSUPPORTED, then the null context: each check before the next, none of them touching a device."""
    fn = getattr(hiplib, entry)
    null = C.c_void_p(None)
    buf = np.zeros(64, np.float64)
    p = C.c_void_p(buf.ctypes.data)
    planes = (p, p, p, p) if entry in DEV else (p, p)
    sz = C.c_size_t

    def call(n, batch, ptrs=planes):
        return fn(null, *ptrs, sz(n), sz(batch), inverse)

    assert call(8, 0) == 0
    assert call(0, 0) == 0  # batch first
    assert call(0, 1) == 1
    assert call((1 << 26) + 1, 1) == -2
    assert call(1 << 27, 1) == -2
    assert call((1 << 25) + 1, 1) == -2  # not a power of two: the Bluestein arm ends at 2^25
    assert call(8, 1) == -3
    assert call(12, 1) == -3             # not a power of two is a valid request
    assert call(1, 1) == -3
    assert call(1 << 26, 1) == -3        # the largest length is a valid request
    assert call(0, 1, (null,) * len(planes)) == 1  # n before the pointers
    assert hiplib.kofft_hip_set_split_fused(null, 0) == -3


def test_python_length_checks_need_no_device(monkeypatch):
    """fft_split / ifft_split / fft_split_complex / fft_complex_vec raise MismatchedLengths (fft.rs:1366, 1394) and the FftPlan forms
    check the plan's length (fft.rs:2081-2112) before any context is created."""
    import kofft_amd as K
    from kofft_amd import api

    def no_device(*a, **k):
        raise AssertionError("a context was created")

    monkeypatch.setattr(api, "HipFftImpl", no_device)
    monkeypatch.setattr(api, "_split_default", {})
    mism = K.FftError(K.FftError.MismatchedLengths)
    for real in (np.float32, np.float64):
        re, im = np.zeros(4, real), np.zeros(3, real)
        for fn in (K.fft_split, K.ifft_split):
            with pytest.raises(K.FftError) as e:
                fn(re, im)
            assert e.value == mism
        for fn in (K.fft_split_complex, K.ifft_split_complex):
            with pytest.raises(K.FftError) as e:
                fn(K.SplitComplex(re, im))  # tests/split.rs:65-74: the struct literal does not compare the lengths
            assert e.value == mism
    with pytest.raises(AssertionError):
        K.SplitComplex.new(np.zeros(4, np.float32), np.zeros(3, np.float32))
    with pytest.raises(AssertionError):
        K.ComplexVec(np.zeros(4, np.float32), np.zeros(3, np.float32))
    with pytest.raises(TypeError):
        K.fft_split(np.zeros(4, np.float32), np.zeros(4, np.float64))

    class NoImpl:
        dtype = np.dtype(np.float32)

        def fft_split(self, *a):
            raise AssertionError("the implementation was called")

        ifft_split = fft_split

    plan = K.FftPlan(16, K.FftStrategy.Auto, NoImpl())
    vec = K.ComplexVec(np.zeros(8, np.float32), np.zeros(8, np.float32))
    for call in (lambda: plan.fft_complex_vec(vec), lambda: plan.ifft_complex_vec(vec), lambda: plan.fft_split(vec.re, vec.im),
                 lambda: plan.ifft_split(vec.re, vec.im), lambda: plan.fft_split(np.zeros(16, np.float32), np.zeros(8, np.float32))):
        with pytest.raises(K.FftError) as e:
            call()
        assert e.value == mism


def test_complex_vec_and_split_complex_round_trip():
    """num.rs:236-308: ComplexVec::from_complex_vec / to_complex_vec / as_slices and SplitComplex::copy_from_complex / copy_to_complex
    keep every bit (-0.0, NaN payloads, subnormals); the types own or view the planes as the reference's do."""
    import kofft_amd as K

    v = np.array([1 - 2j, complex(-0.0, 1e-45), complex(np.inf, -np.nan), 3.5 + 0j], np.complex64)
    cv = K.ComplexVec.from_complex_vec(v)
    assert cv.len() == len(cv) == 4 and not cv.is_empty()
    re, im = cv.as_slices()
    assert re.dtype == im.dtype == np.float32
    assert bits_equal(re, np.ascontiguousarray(v.real)) and bits_equal(im, np.ascontiguousarray(v.imag))
    assert bits_equal(cv.to_complex_vec(), v)
    assert cv == K.ComplexVec(re, im) and cv != K.ComplexVec(im, re)
    src = np.arange(4, dtype=np.float32)
    own = K.ComplexVec(src, src)
    src[0] = 9
    assert own.re[0] == 0  # owned, like Vec<f32>
    assert K.ComplexVec([], []).is_empty()
    for cdt, real in ((np.complex64, np.float32), (np.complex128, np.float64)):
        z = v.astype(cdt)
        r, i = np.zeros(4, real), np.zeros(4, real)
        sc = K.SplitComplex.copy_from_complex(z, r, i)
        assert sc.re is r and sc.im is i and sc.len() == 4 and not sc.is_empty()  # a view of the caller's planes
        back = np.zeros(4, cdt)
        sc.copy_to_complex(back)
        assert bits_equal(back, z)


@pytest.mark.parametrize("real", [np.float32, np.float64])
@pytest.mark.parametrize("n", [32, 64, 1024])
def test_split_oracle_agrees_with_restated_stages(oracle, real, n):
    """tests/split_oracle.py (the C oracle's complex transform on the joined planes) against the stages of fft_split_simd restated on two
    numpy planes (ref_restatement._stockham, fft.rs:834-898 / 959-1037) with the restated table, bit for bit; the inverse against
    ifft_split's own loop around them (fft.rs:1400-1409)."""
    rng = seeded(8800 + n)
    re, im = rng.uniform(-1, 1, n).astype(real), rng.uniform(-1, 1, n).astype(real)
    tw = rr.get_twiddles(n, real)
    wr, wi = rr._stockham(re.copy(), im.copy(), tw)
    gr, gi = split_ref(re, im)
    assert gr.dtype == real and bits_equal(gr, wr) and bits_equal(gi, wi)
    ir, ii = rr._stockham(re.copy(), -im, tw)
    scale = real(1.0) / real(np.float32(n))
    ii = -ii
    ir, ii = ir * scale, ii * scale
    gr, gi = split_ref(re, im, inverse=True)
    assert bits_equal(gr, ir.astype(real)) and bits_equal(gi, ii.astype(real))


def test_split_oracle_shapes_and_identity(oracle):
    """[batch, n] planes transform row by row; n == 1 is the identity in both directions."""
    rng = seeded(8899)
    re, im = rng.uniform(-1, 1, (3, 12)).astype(np.float32), rng.uniform(-1, 1, (3, 12)).astype(np.float32)
    gr, gi = split_ref(re, im)
    for b in range(3):
        r1, i1 = split_ref(re[b], im[b])
        assert bits_equal(gr[b], r1) and bits_equal(gi[b], i1)
    one_r, one_i = np.array([[3.5], [-0.0]], np.float64), np.array([[-1e-310], [np.inf]], np.float64)
    for inverse in (False, True):
        gr, gi = split_ref(one_r, one_i, inverse)
        assert bits_equal(gr, one_r) and bits_equal(gi, one_i)


def test_every_new_entry_has_a_guard_band_case():
    """The device-pointer forms are named kofft_hip_dev_* like the chirp-Z ones: tests/test_redzone.py matches every *_dev name of the
    header against the case table of tests/test_gpu_footprint.py, which predates these calls.  Their guard-band cases, and the host
    forms', are in tests/test_gpu_split.py: every declared entry of the family is called there inside an arena."""
    from pathlib import Path

    from kofft_amd import _lib

    family = [s for s in _lib.header_symbols() if "fft_split" in s and s != "kofft_hip_set_split_fused"]
    assert sorted(family) == sorted(HOST + DEV)
    assert not [s for s in family if s.endswith("_dev")]
    src = (Path(__file__).resolve().parent / "test_gpu_split.py").read_text()
    body = src[src.index("def test_split_guard_bands"):src.index("def test_split_dev_on_a_side_stream")]
    assert 'f"dev_fft_split_{stem}"' in body and 'f"fft_split_{stem}"' in body and "arena.verify()" in body
