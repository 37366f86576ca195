"""dct::dct1..dct4 / dst::dst1..dst4 on the device, bit for bit against tests/trig_direct_oracle.py.  The tiled kernel
(direct_tiled_kernel<M>, n >= 64 and batch >= 64) and the simple kernel (direct_simple_kernel<M>: every other shape, and every
shape in a context with set_direct_tiled(False)) must agree byte for byte on every output; the oracle checks every output of every
row: the numpy restatement for n <= 256, the C restatement (oracle/kofft_oracle.c: ko_direct_f32, checked against the numpy one on CPU
by tests/test_trig_direct_cpu.py) beyond."""
import numpy as np
import pytest

from conftest import bits_equal, seeded
from rowcheck import assert_rows_equal
from trig_direct_oracle import KINDS, direct

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 4, 5, 7, 8, 16, 31, 32, 33, 40, 63, 64, 100, 127, 128, 255, 256, 500, 512, 1000, 1023, 1024, 2048, 4095, 4096]
TILE = 128  # DT_BM: rows of one tiled workgroup
BATCHES = [1, 3, TILE - 1, TILE, TILE + 1, 300]


@pytest.fixture(scope="module")
def simple32():
    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    f.set_direct_tiled(False)
    return f


def _run(f, family, type, x):
    fn = f.dct_direct_batch if family == "dct" else f.dst_direct_batch
    a = fn(x, type)
    b = fn(x, type)
    assert bits_equal(a, b), f"{family}{type}: two runs of the same call differ"
    return a


def _nan_safe_equal(got, want):
    ng, nw = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(ng, nw) and got[~ng].tobytes() == want[~nw].tobytes()


def _check_oracle(got, family, type, x, what, nan_safe=False):
    """Every output of every row against the oracle."""
    from oracle import pyoracle

    want = direct(family, type, x) if x.shape[1] <= 256 else pyoracle.direct_mt(family, type, x)
    assert_rows_equal(got, want, what, nan_safe=nan_safe)


@pytest.mark.parametrize("family,type", KINDS)
@pytest.mark.parametrize("n", NS)
def test_bit_exact_and_tiled_equals_simple(fft32, simple32, family, type, n):
    for batch in BATCHES:
        seed = 12000 + 31 * n + 7 * batch + 3 * type + (500 if family == "dst" else 0)
        x = seeded(seed).uniform(-1, 1, (batch, n)).astype(np.float32)
        got = _run(fft32, family, type, x)
        assert bits_equal(got, _run(simple32, family, type, x)), f"{family}{type} n={n} batch={batch}: tiled != simple"
        _check_oracle(got, family, type, x, f"{family}{type} n={n} batch={batch}")


def _special_rows(n, rng):
    rows = [np.full(n, -0.0, np.float32), np.full(n, 0.0, np.float32)]
    specials = np.array([np.float32(1e-45), -np.float32(1e-45), np.float32(1.2e-38), np.float32(3e38), -np.float32(3e38),
                         np.inf, -np.inf, np.nan, 0.0, -0.0], np.float32)
    for j in range(6):
        r = rng.uniform(-1, 1, n).astype(np.float32)
        pos = rng.choice(n, size=min(n, 1 + j), replace=False)
        r[pos] = rng.choice(specials, size=pos.size)
        rows.append(r)
    rows.append(np.full(n, 3e38, np.float32))  # DCT-I's 2 * x overflows
    sub = np.full(n, 1e-40, np.float32)
    sub[0] = -1e-41
    rows.append(sub)
    return np.stack(rows)


@pytest.mark.parametrize("family,type", KINDS)
@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 130, 256, 1024])
def test_special_values(fft32, simple32, family, type, n):
    rng = seeded(13000 + n + type)
    x = _special_rows(n, rng)
    x = np.concatenate([x] * (1 + 140 // x.shape[0]))[:max(x.shape[0], 140)]  # >= 64 rows: the tiled kernel runs at n >= 64
    got = _run(fft32, family, type, x)
    assert _nan_safe_equal(got, _run(simple32, family, type, x))
    _check_oracle(got, family, type, x, f"{family}{type} n={n} specials", nan_safe=True)
    if not (family == "dct" and type == 1) and type != 3:
        assert bits_equal(got[0], np.zeros(n, np.float32)), "an all -0 row gives +0 (the +0.0 seed)"


def test_host_form_in_place_and_dev_form(fft32):
    import torch

    rng = seeded(14000)
    for family, type in KINDS:
        for n, batch in [(33, 5), (256, 200)]:
            x = rng.uniform(-1, 1, (batch, n)).astype(np.float32)
            want = _run(fft32, family, type, x)
            buf = x.copy()
            fn = fft32._lib.kofft_hip_dct_direct_f32 if family == "dct" else fft32._lib.kofft_hip_dst_direct_f32
            fft32._check(fn(fft32._ctx, type, buf.ctypes.data, buf.ctypes.data, n, batch))  # in == out
            assert bits_equal(buf, want)
            d_in = torch.from_numpy(x).cuda()
            d_out = torch.empty_like(d_in)
            dev = fft32.dct_direct_dev if family == "dct" else fft32.dst_direct_dev
            dev(type, d_in.data_ptr(), d_out.data_ptr(), n, batch)
            torch.cuda.synchronize()
            assert bits_equal(d_out.cpu().numpy(), want)
    import kofft_amd

    d = torch.zeros(4 * 64, device="cuda")
    with pytest.raises(kofft_amd.FftError):  # overlapping device buffers
        fft32.dct_direct_dev(2, d.data_ptr(), d.data_ptr() + 4 * 8, 64, 3)


def test_python_modules(fft32):
    from kofft_amd import dct, dst

    rng = seeded(15000)
    for mod, family in ((dct, "dct"), (dst, "dst")):
        for type in (1, 2, 3, 4):
            x1 = rng.uniform(-1, 1, 40).astype(np.float32)
            one = getattr(mod, f"{family}{type}")(x1)
            assert one.shape == (40,) and bits_equal(one, direct(family, type, x1[None])[0])
            x2 = rng.uniform(-1, 1, (3, 40)).astype(np.float32)
            assert bits_equal(getattr(mod, f"{family}{type}")(x2, fft=fft32), _run(fft32, family, type, x2))
            rows = [rng.uniform(-1, 1, m).astype(np.float32) for m in (5, 64, 5, 1, 300, 64, 0 if type != 3 else 2)]
            want = [direct(family, type, r[None])[0] for r in rows]
            name = {1: "i", 2: "ii", 3: "iii", 4: "iv"}[type]
            getattr(mod, f"batch_{name}")(rows)
            for r, w in zip(rows, want):
                assert bits_equal(r, w)
            chans = [rng.uniform(-1, 1, 16).astype(np.float32) for _ in range(2)]
            want = [direct(family, type, r[None])[0] for r in chans]
            getattr(mod, f"multi_channel_{name}")(chans, fft=fft32)
            assert all(bits_equal(r, w) for r, w in zip(chans, want))


def test_naive_dct2_is_not_plan_dct2_but_close(fft32, oracle):
    """kofft_hip_dct_direct_f32(.., 2, ..) is dct::dct2; dct2_batch is plan_dct2 -- within 1e-4 on dct.rs:183-195's input."""
    x = np.array([[1.0, 2.0, 3.0, 4.0]], np.float32)
    assert np.all(np.abs(fft32.dct_direct_batch(x, 2) - fft32.dct2_batch(x)) < 1e-4)
