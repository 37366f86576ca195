"""FftImpl::fft_split / ifft_split (fft.rs:1365-1439) on the device, bit for bit against tests/split_oracle.py.  Powers of two 2 .. 2^14
(f32) / 2^13 (f64) run PlanarIO in fft_small_kernel / fft_wg_kernel on the planes themselves (one launch); every other length -- and every
length in a context with set_split_fused(False) -- runs planar_pack_kernel -> fft_dev (in place, in the context's scratch) ->
planar_unpack_kernel.  n == 1 copies the planes."""
import numpy as np
import pytest

from conftest import bits_equal, seeded
from redzone import Arena
from rowcheck import assert_rows_equal
from split_oracle import split_ref

pytestmark = pytest.mark.gpu

REALS = [np.float32, np.float64]
MAX_LOG2 = {np.float32: 14, np.float64: 13}  # host_common.hip.h: max_log2<T>()
POW2_CASES = [(real, l) for real in REALS for l in range(0, MAX_LOG2[real] + 1)]


def _id(case):
    return f"{np.dtype(case[0]).name}-2^{case[1]}"


@pytest.fixture(scope="module")
def num_cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def composed():
    """Contexts with the fused route off (set_split_fused(False)): every planar transform through pack, fft_dev, unpack."""
    import kofft_amd

    ctx = {}
    for real in REALS:
        ctx[real] = kofft_amd.HipFftImpl(real)
        ctx[real].set_split_fused(False)
    return ctx


@pytest.fixture(scope="module")
def default(fft32, fft64):
    return {np.float32: fft32, np.float64: fft64}


def _planes(seed, shape, real):
    rng = seeded(seed)
    return rng.uniform(-1, 1, shape).astype(real), rng.uniform(-1, 1, shape).astype(real)


def _twice(f, re, im, inverse):
    """fft_split_batch (in place) on two copies of the same planes: the two runs must give the same bytes."""
    a, b = (re.copy(), im.copy()), (re.copy(), im.copy())
    f.fft_split_batch(a[0], a[1], inverse)
    f.fft_split_batch(b[0], b[1], inverse)
    assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1]), "fft_split_batch: two runs of the same call differ"
    return a


def _check(f, re, im, inverse, what, nan_safe=False):
    got = _twice(f, re, im, inverse)
    want = split_ref(re, im, inverse)
    assert_rows_equal(got[0], want[0], what + " re", nan_safe=nan_safe)
    assert_rows_equal(got[1], want[1], what + " im", nan_safe=nan_safe)
    return got


def _dev(f, re, im, inverse, in_place=False, offset=0):
    """fft_split_dev on device copies of the planes; offset: elements into a larger allocation (element alignment only)."""
    import torch

    def up(a):
        d = torch.empty(a.size + offset, dtype=torch.from_numpy(a).dtype, device="cuda")
        d[offset:] = torch.from_numpy(a.reshape(-1)).cuda()
        return d[offset:].view(a.shape)

    d_re, d_im = up(re), up(im)
    torch.cuda.synchronize()  # the slice assignments above are copies on torch's stream; the context's own stream does not wait for it
    if in_place:
        o_re, o_im = f.fft_split_dev(d_re, d_im, inverse=inverse)
        assert o_re is d_re and o_im is d_im
    else:
        o_re, o_im = up(np.zeros_like(re)), up(np.zeros_like(im))
        torch.cuda.synchronize()
        f.fft_split_dev(d_re, d_im, o_re, o_im, inverse=inverse)
    f.synchronize()
    if not in_place:
        assert bits_equal(d_re.cpu().numpy(), re) and bits_equal(d_im.cpu().numpy(), im), "an input plane changed"
    return o_re.cpu().numpy(), o_im.cpu().numpy()


@pytest.mark.parametrize("case", POW2_CASES, ids=_id)
def test_split_pow2_ladder(default, oracle, case):
    """Every power of two n = 1 .. 2^14 (f64: 2^13), forward and inverse, at batches 1, 3 and 33 (the tile kernel's last workgroup
    partly filled: it takes 256 / (n >> rl_for) rows), each call twice."""
    real, log2n = case
    n = 1 << log2n
    for batch in (1, 3, 33):
        for inverse in (False, True):
            re, im = _planes(9000 + 37 * log2n + batch, (batch, n), real)
            _check(default[real], re, im, inverse, f"n={n} batch={batch} inverse={inverse}")


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("n", [1 << 15, 1 << 16, 3, 12, 15, 1000, 4097])
def test_split_composed_lengths(default, oracle, real, n):
    """Lengths the fused route does not take: powers of two above 2^14 / 2^13 and lengths that are not a power of two (Bluestein), in the
    default context, batches 1 and 3, both directions."""
    for batch in (1, 3):
        for inverse in (False, True):
            re, im = _planes(9100 + n + batch, (batch, n), real)
            _check(default[real], re, im, inverse, f"n={n} batch={batch} inverse={inverse}")


def test_split_composed_reaches_persistent_kernel(composed, oracle, num_cus):
    """n = 1024 in f32 just above the complex transform's persistent threshold (host_common.hip.h: dispatch, L == 10: 32 rows per CU,
    restated here as test_gpu_hilbert.py does): the composed route hands fft_dev the whole batch."""
    n, batch = 1024, 32 * num_cus + 1
    re, im = _planes(9200, (batch, n), np.float32)
    _check(composed[np.float32], re, im, False, f"n={n} batch={batch}")


@pytest.mark.parametrize("case", [c for c in POW2_CASES if c[1] >= 1], ids=_id)
def test_split_fused_equals_composed(default, composed, oracle, case):
    """n = 2 .. 2^14 (f64: 2^13): the fused route and the composed route give the same bytes, at batches 1, 5, 33, both directions."""
    real, log2n = case
    n = 1 << log2n
    for batch in (1, 5, 33):
        for inverse in (False, True):
            re, im = _planes(9300 + 41 * log2n + batch, (batch, n), real)
            what = f"n={n} batch={batch} inverse={inverse}"
            fused = _check(default[real], re, im, inverse, what)
            other = _twice(composed[real], re, im, inverse)
            assert bits_equal(fused[0], other[0]) and bits_equal(fused[1], other[1]), what


@pytest.mark.parametrize("real", REALS)
def test_split_dev_layouts(default, composed, oracle, real):
    """Device planes on both routes: in place (the outputs are the inputs) and out of place give the oracle's bytes, out of place
    leaves the inputs as they were, and planes one element into an allocation (4- / 8-byte aligned only) work."""
    for n, batch in [(1, 6), (8, 5), (32, 9), (64, 40), (1024, 7), (4096, 3), (8192, 3), (1000, 3), (1 << 15, 2)]:
        for inverse in (False, True):
            re, im = _planes(9400 + n, (batch, n), real)
            want = split_ref(re, im, inverse)
            for f in (default[real], composed[real]):
                for in_place, offset in [(False, 0), (True, 0), (False, 1), (True, 1)]:
                    got = _dev(f, re, im, inverse, in_place, offset)
                    what = f"n={n} batch={batch} inverse={inverse} in_place={in_place} offset={offset}"
                    assert_rows_equal(got[0], want[0], what + " re")
                    assert_rows_equal(got[1], want[1], what + " im")


@pytest.mark.parametrize("real", REALS)
def test_split_host_equals_dev(default, composed, oracle, real):
    """The host entry and the device entry give the same bytes at sizes that go zero-copy (planes up to 512 KiB) and staged; 1-D
    planes through fft_split / ifft_split as well."""
    for f in (default[real], composed[real]):
        for n, batch in [(8, 5), (256, 100), (1024, 300), (12, 7), (1 << 16, 3)]:
            for inverse in (False, True):
                re, im = _planes(9500 + n, (batch, n), real)
                host = _check(f, re, im, inverse, f"n={n} batch={batch} inverse={inverse}")
                dev = _dev(f, re, im, inverse)
                assert bits_equal(host[0], dev[0]) and bits_equal(host[1], dev[1]), f"n={n} batch={batch}"
        re, im = _planes(9550, 64, real)
        want = split_ref(re, im)
        f.fft_split(re, im)
        assert bits_equal(re, want[0]) and bits_equal(im, want[1])
        back = split_ref(re, im, True)
        f.ifft_split(re, im)
        assert bits_equal(re, back[0]) and bits_equal(im, back[1])


@pytest.mark.parametrize("real", REALS)
def test_split_equals_interleaved(default, oracle, real):
    """The reference's own property (tests/split.rs, split64.rs), bit for bit: the planar result is fft_batch's on the interleaved
    data, both directions."""
    f = default[real]
    for n, batch in [(12, 3), (16, 5), (32, 5), (64, 7), (1024, 33), (4097, 2), (1 << 14, 2), (1 << 15, 2)]:
        for inverse in (False, True):
            re, im = _planes(9600 + n, (batch, n), real)
            z = np.empty((batch, n), np.complex64 if real == np.float32 else np.complex128)
            z.real, z.imag = re, im
            f.fft_batch(z, inverse)
            f.fft_split_batch(re, im, inverse)
            what = f"n={n} inverse={inverse}"
            assert_rows_equal(re, np.ascontiguousarray(z.real), what + " re")
            assert_rows_equal(im, np.ascontiguousarray(z.imag), what + " im")


@pytest.mark.parametrize("real", REALS)
@pytest.mark.parametrize("n", [2, 8, 32, 64, 1024, 4096, 1 << 15])
def test_split_special_values(default, composed, oracle, real, n):
    """+-0, subnormals, values near the largest finite one, +-Inf and NaN go through the same operations as in the reference on both
    routes and in both directions: NaNs in the same places, every other value (-0.0 and subnormal outputs included) the same bits."""
    tiny, big = (1e-45, 3e38) if real == np.float32 else (5e-324, 1.7e308)
    specials = np.array([0.0, -0.0, tiny, -tiny, np.finfo(real).tiny, big, -big, np.inf, -np.inf, np.nan, 1.0, -3.5], real)
    rng = seeded(9700 + n)
    rows_re, rows_im = [], []
    for i in range(len(specials) + 2):
        r, m = rng.uniform(-1, 1, n).astype(real), rng.uniform(-1, 1, n).astype(real)
        if i < len(specials):
            (r if i % 2 else m)[rng.integers(0, n)] = specials[i]
        elif i == len(specials):
            r[:] = specials[rng.integers(0, len(specials), n)]
            m[:] = specials[rng.integers(0, len(specials), n)]
        else:
            r[:] = real(-0.0)
            m[:] = real(-0.0)
        rows_re.append(r)
        rows_im.append(m)
    re, im = np.stack(rows_re), np.stack(rows_im)
    assert np.isnan(split_ref(re, im)[0]).any()
    for f in (default[real], composed[real]):
        for inverse in (False, True):
            _check(f, re, im, inverse, f"n={n} inverse={inverse}", nan_safe=True)


@pytest.mark.parametrize("real", REALS)
def test_split_length_one_is_identity(default, composed, real):
    """n == 1, both directions, host and device entries, both contexts: the planes are unchanged, bit for bit (-0.0, subnormals, Inf)."""
    tiny = 1e-45 if real == np.float32 else 5e-324
    re = np.array([[3.5], [-0.0], [tiny], [np.inf], [-2.0]], real)
    im = np.array([[-0.0], [1.25], [-np.inf], [-tiny], [0.0]], real)
    for f in (default[real], composed[real]):
        for inverse in (False, True):
            got = _twice(f, re, im, inverse)
            assert bits_equal(got[0], re) and bits_equal(got[1], im)
            for in_place in (False, True):
                got = _dev(f, re, im, inverse, in_place)
                assert bits_equal(got[0], re) and bits_equal(got[1], im)


@pytest.mark.parametrize("real", REALS)
def test_split_guard_bands(default, composed, oracle, real):
    """tests/redzone.py around the planes: the device entries and the host entries write only their two output planes; with distinct
    outputs the device entries leave their inputs untouched.  Both routes, a row length that is not a multiple of any tile, a partly
    filled last workgroup and planes that are element-aligned only."""
    item = np.dtype(real).itemsize
    stem = "c32" if real == np.float32 else "c64"
    for f in (default[real], composed[real]):
        for n, batch in [(1, 5), (4, 3), (16, 257), (32, 33), (256, 9), (1024, 5), (8192, 2), (1000, 3), (1 << 15, 1)]:
            for inverse in (0, 1):
                re, im = _planes(9800 + n, (batch, n), real)
                want = split_ref(re, im, bool(inverse))
                what = f"fft_split_{stem} n={n} batch={batch} inverse={inverse}"
                # device, out of place
                arena = Arena("cuda", what + " dev oop")
                a_re, a_im = arena.input(re, item, n * item, "re_in"), arena.input(im, 0, n * item, "im_in")
                o_re, o_im = arena.output(re.nbytes, 0, None, n * item, "re_out"), arena.output(im.nbytes, item, None, n * item, "im_out")
                f._check(f._fn(f"dev_fft_split_{stem}")(f._ctx, a_re.addr, a_im.addr, o_re.addr, o_im.addr, n, batch, inverse))
                f.synchronize()
                arena.verify()
                assert bits_equal(arena.read(o_re, real, (batch, n)), want[0]) and bits_equal(arena.read(o_im, real, (batch, n)), want[1]), what
                # device, in place
                arena = Arena("cuda", what + " dev in place")
                a_re, a_im = arena.inout(re, 0, n * item, "re"), arena.inout(im, item, n * item, "im")
                f._check(f._fn(f"dev_fft_split_{stem}")(f._ctx, a_re.addr, a_im.addr, a_re.addr, a_im.addr, n, batch, inverse))
                f.synchronize()
                arena.verify()
                assert bits_equal(arena.read(a_re, real, (batch, n)), want[0]) and bits_equal(arena.read(a_im, real, (batch, n)), want[1]), what
                # host (in place)
                arena = Arena("host", what + " host")
                a_re, a_im = arena.inout(re, item, n * item, "re"), arena.inout(im, 0, n * item, "im")
                f._check(f._fn(f"fft_split_{stem}")(f._ctx, a_re.addr, a_im.addr, n, batch, inverse))
                arena.verify()
                assert bits_equal(arena.read(a_re, real, (batch, n)), want[0]) and bits_equal(arena.read(a_im, real, (batch, n)), want[1]), what


def test_split_dev_on_a_side_stream(oracle):
    """A _dev call after set_stream on a caller's stream, both routes: the oracle's bytes."""
    import torch

    import kofft_amd

    side = torch.cuda.Stream()
    for fused in (True, False):
        f = kofft_amd.HipFftImpl(np.float32)
        f.set_split_fused(fused)
        f.set_stream(side.cuda_stream)
        for n, batch in [(1024, 9), (1000, 3), (1, 4), (1 << 15, 2)]:
            re, im = _planes(9900 + n, (batch, n), np.float32)
            want = split_ref(re, im)
            with torch.cuda.stream(side):
                d_re, d_im = torch.from_numpy(re).cuda(), torch.from_numpy(im).cuda()
                o_re, o_im = torch.empty_like(d_re), torch.empty_like(d_im)
                f.fft_split_dev(d_re, d_im, o_re, o_im)
            side.synchronize()
            assert bits_equal(o_re.cpu().numpy(), want[0]) and bits_equal(o_im.cpu().numpy(), want[1]), f"n={n} fused={fused}"
        f.set_stream(0)
        f.close()


def test_split_n32_on_the_workgroup_kernel(oracle, monkeypatch):
    """KOFFT_HIP_SMALL32=0 (read when the context is created): f32 n = 32 runs fft_wg_kernel<5> instead of one thread per transform --
    the same bytes."""
    import kofft_amd

    monkeypatch.setenv("KOFFT_HIP_SMALL32", "0")
    f = kofft_amd.HipFftImpl(np.float32)
    for batch in (1, 33, 300):
        for inverse in (False, True):
            re, im = _planes(9950 + batch, (batch, 32), np.float32)
            _check(f, re, im, inverse, f"n=32 batch={batch} inverse={inverse}")
    f.close()


def test_split_reference_pins(fft32, fft64, oracle):
    """tests/split.rs and tests/split64.rs restated: the SoA entries against the AoS ones (n = 16 and 32, the non-power-of-two n = 12),
    the n = 64 round trips (1e-4 in f32, 1e-8 in f64), ComplexVec's round trip at n = 32 and the length error."""
    import kofft_amd as K

    for n in (16, 12):  # split.rs:11-44
        data = np.arange(n).astype(np.complex64)
        re, im = np.zeros(n, np.float32), np.zeros(n, np.float32)
        split = K.SplitComplex.copy_from_complex(data, re, im)
        aos = data.copy()
        fft32.fft(aos)
        K.fft_split_complex(split, fft32)
        assert np.all(np.abs(aos.real - re) < 1e-6) and np.all(np.abs(aos.imag - im) < 1e-6)
    for n in (32, 12):  # split64.rs:3-34
        aos = np.arange(n).astype(np.complex128)
        re, im = np.arange(n, dtype=np.float64), np.zeros(n)
        fft64.fft(aos)
        K.fft_split(re, im, fft64)
        assert np.all(np.abs(aos.real - re) < 1e-10) and np.all(np.abs(aos.imag - im) < 1e-10)
    n = 64  # split.rs:46-63, split64.rs:36-50
    for real, f, tol in ((np.float32, fft32, 1e-4), (np.float64, fft64, 1e-8)):
        re, im = np.arange(n, dtype=real), -np.arange(n, dtype=real)
        K.fft_split_complex(K.SplitComplex(re, im), f)
        K.ifft_split_complex(K.SplitComplex(re, im), f)
        assert np.all(np.abs(re - np.arange(n)) < tol) and np.all(np.abs(im + np.arange(n)) < tol)
    with pytest.raises(K.FftError) as e:  # split.rs:65-74
        K.fft_split_complex(K.SplitComplex(np.zeros(4, np.float32), np.zeros(3, np.float32)), fft32)
    assert e.value == K.FftError(K.FftError.MismatchedLengths)
    data = (np.arange(32) - 1j * np.arange(32)).astype(np.complex64)  # split.rs:76-93
    vec = K.ComplexVec.from_complex_vec(data)
    K.fft_complex_vec(vec, fft32)
    assert bits_equal(vec.to_complex_vec(), oracle.fft(data))
    K.ifft_complex_vec(vec, fft32)
    assert np.all(np.abs(vec.re - data.real) < 1e-4) and np.all(np.abs(vec.im - data.imag) < 1e-4)
    plan = K.FftPlan(32, K.FftStrategy.Auto, fft32)
    vec = K.ComplexVec.from_complex_vec(data)
    plan.fft_complex_vec(vec)
    assert bits_equal(vec.to_complex_vec(), oracle.fft(data))
    plan.ifft_complex_vec(vec)
    assert bits_equal(vec.to_complex_vec(), oracle.ifft(oracle.fft(data)))
    K.fft_split(np.arange(8, dtype=np.float32), np.zeros(8, np.float32))  # the free function's own default context


def test_split_errors(fft32, fft64):
    """n = 0 -> EmptyInput; mismatched planes -> MismatchedLengths; n beyond 2^26 -> KOFFT_ERR_UNSUPPORTED; batch 0 -> nothing to do;
    planes of the wrong precision or shape are refused by the batched methods; planes that are not contiguous arrays of the context's
    precision still transform through fft_split (as before this entry existed)."""
    import torch

    import kofft_amd as K

    with pytest.raises(K.FftError) as e:
        fft32.fft_split(np.zeros(0, np.float32), np.zeros(0, np.float32))
    assert e.value == K.FftError(K.FftError.EmptyInput)
    with pytest.raises(K.FftError) as e:
        fft32.fft_split_batch(np.zeros((2, 4), np.float32), np.zeros((2, 3), np.float32))
    assert e.value == K.FftError(K.FftError.MismatchedLengths)
    with pytest.raises(K.DeviceError) as d:
        fft32._check(fft32._lib.kofft_hip_dev_fft_split_c32(fft32._ctx, 0, 0, 0, 0, 1 << 27, 1, 0))
    assert d.value.code == -2
    fft32.fft_split_batch(np.zeros((0, 8), np.float32), np.zeros((0, 8), np.float32))
    with pytest.raises(TypeError):
        fft32.fft_split_batch(np.zeros((1, 8), np.float64), np.zeros((1, 8), np.float64))
    with pytest.raises(TypeError):
        fft64.fft_split_batch(np.zeros(8), np.zeros(8))
    with pytest.raises(TypeError):
        fft32.fft_split_dev(torch.zeros(8, dtype=torch.float64, device="cuda"), torch.zeros(8, dtype=torch.float64, device="cuda"))
    with pytest.raises(K.FftError):
        fft32.fft_split_dev(torch.zeros(8, device="cuda"), torch.zeros(4, device="cuda"))
    wide = np.zeros((8, 2), np.float32)
    wide[:, 0] = np.arange(8)
    re, im = wide[:, 0], np.zeros(8, np.float64)  # a strided f32 plane and an f64 plane in an f32 context
    fft32.fft_split(re, im)
    want = split_ref(np.arange(8, dtype=np.float32), np.zeros(8, np.float32))
    assert bits_equal(np.ascontiguousarray(re), want[0]) and bits_equal(im.astype(np.float32), want[1])
