"""Polyphase resampling of rows on the device, bit for bit against tests/resample_oracle.py.  A default context runs
resample_tiled_kernel wherever kofft_hip_resample_route says 1 and resample_plain_kernel elsewhere; a context with
set_resample_tiled(False) runs the plain kernel always.  Every call runs twice and its two results are compared; both contexts get the
same inputs and must give the same bytes."""
import re

import numpy as np
import pytest

from conftest import bits_equal, seeded
from resample_oracle import forward_bound, full_len, resample_ref
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32


def _tile():
    from kofft_amd import _lib

    return int(re.search(r"#define KOFFT_HIP_RESAMPLE_TILE (\d+)", _lib.HEADER_PATH.read_text()).group(1))


T = _tile()  # the most outputs of one workgroup tile of the tiled kernel (4 x 255 at 3 / 1, 4 x 252 at 7 / 5)


@pytest.fixture(scope="module")
def plain32():
    """A context with the tiled route off (set_resample_tiled(False)): every call on the plain kernel."""
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_resample_tiled(False)
    yield f
    f.close()


def _route(nh, up, down):
    from kofft_amd import resample

    return resample.route(nh, up, down)


def _rand(seed, rows, nx, nh):
    rng = seeded(seed)
    return rng.uniform(-1, 1, (rows, nx)).astype(F), rng.uniform(-1, 1, nh).astype(F)


def _host(f, x, h, up, down, t0, out_len, off=0):
    a = f.resample_rows(x, h, up, down, t0, out_len)
    b = f.resample_rows(x, h, up, down, t0, out_len)
    assert bits_equal(a, b), "resample_rows: two runs of the same call differ"
    return a


def _dev(f, x, h, up, down, t0, out_len, off=0):
    """The device entry on torch buffers, twice; off: floats by which x, h and the output are shifted into their allocations."""
    import torch

    rows, nx = x.shape
    dx = torch.zeros(x.size + off, dtype=torch.float32, device="cuda")
    dx[off:] = torch.from_numpy(x.reshape(-1)).cuda()
    dh = torch.zeros(h.size + off, dtype=torch.float32, device="cuda")
    dh[off:] = torch.from_numpy(h).cuda()
    res = []
    for _ in range(2):
        out = torch.full((rows * out_len + off,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # (torch's copies and fills run on its stream, the call on the context's own)
        f.resample_dev(dx.data_ptr() + 4 * off, rows, nx, dh.data_ptr() + 4 * off, h.size, up, down, t0, out.data_ptr() + 4 * off, out_len)
        f.synchronize()
        res.append(out[off:].cpu().numpy().reshape(rows, out_len))
    assert bits_equal(res[0], res[1]), "resample_dev: two runs of the same call differ"
    return res[0]


def _both(fft32, plain32, x, h, up, down, t0, out_len, what, want=None, nan_safe=False, run=_host, off=0):
    if want is None:
        want = resample_ref(x, h, up, down, t0, out_len)
    got = run(fft32, x, h, up, down, t0, out_len, off)
    assert_rows_equal(got, want, what + ": default route", nan_safe=nan_safe)
    got_p = run(plain32, x, h, up, down, t0, out_len, off)
    assert_rows_equal(got_p, want, what + ": plain route", nan_safe=nan_safe)
    assert_rows_equal(got, got_p, what + ": the two routes differ", nan_safe=nan_safe)
    return got


@pytest.mark.parametrize("up,down", [(1, 1), (1, 2), (1, 3), (2, 1), (3, 1), (3, 2), (2, 3), (4, 2), (7, 5), (160, 441), (441, 160)])
def test_rate_ladder(fft32, plain32, up, down):
    """nh = 4 max(up, down) + 1, three rows, 2 T + 5 outputs per row from time 0: three tiles per row, the last one short.  nx is
    the smallest whose full result has that many outputs (with up > down the full lengths skip values: then the first 2 T + 5)."""
    nh = 4 * max(up, down) + 1
    out_len = 2 * T + 5
    nx = 1
    while full_len(nx, nh, up, down) < out_len:
        nx += 1
    assert full_len(nx, nh, up, down) - out_len < -(-up // down) and _route(nh, up, down) == 1
    x, h = _rand(27200 + 7 * up + down, 3, nx, nh)
    want = resample_ref(x, h, up, down, 0, out_len)
    what = f"up={up} down={down} nx={nx} nh={nh}"
    _both(fft32, plain32, x, h, up, down, 0, out_len, what, want)
    _both(fft32, plain32, x, h, up, down, 0, out_len, what + " dev", want, run=_dev)


@pytest.mark.parametrize("up,down", [(1, 1), (1, 2), (1, 3), (2, 1), (4, 2), (256, 3), (3, 1)])
def test_row_ends_inside_a_full_tile(fft32, plain32, up, down):
    """T - 24 .. T + 300 outputs per row with 61 taps and more: the outputs that run off the row's end sit in the last quarter of a
    full tile or in a short second one, so a thread of the kernel instance that sums four outputs of one phase at a time (256 down a
    multiple of up: every pair here but 3 / 1) holds outputs with different term ranges, and threads with fewer than four outputs."""
    nh = 61 if up < 61 else 4 * up + 1
    for target in (T - 24, T, T + 300):
        nx = 1
        while full_len(nx, nh, up, down) < target:
            nx += 1
        out_len = full_len(nx, nh, up, down)
        assert _route(nh, up, down) == 1 and target <= out_len < target + -(-up // down)
        x, h = _rand(27250 + up + down + target, 3, nx, nh)
        _both(fft32, plain32, x, h, up, down, 0, out_len, f"row ends up={up} down={down} nx={nx} out_len={out_len}", run=_dev)


LADDER_NH = [1, 2, 3, 31, 257, 4097, 20001]


def test_filter_ladder_holds_both_routes():
    routes = [_route(nh, 3, 2) for nh in LADDER_NH]
    assert 0 in routes and 1 in routes, routes


@pytest.mark.parametrize("nh", LADDER_NH)
def test_filter_ladder(fft32, plain32, nh):
    up, down, nx = 3, 2, 700
    x, h = _rand(27300 + nh, 3, nx, nh)
    out_len = full_len(nx, nh, up, down)
    _both(fft32, plain32, x, h, up, down, 0, out_len, f"3/2 nx={nx} nh={nh} route={_route(nh, up, down)}")


@pytest.mark.parametrize("up,down", [(3, 2), (1, 3)])
def test_route_seam(fft32, plain32, up, down):
    """The largest nh the tiled kernel takes, found by bisection on the query (monotone in nh), and the one after it."""
    lo, hi = 1, 1 << 20
    assert _route(lo, up, down) == 1 and _route(hi, up, down) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _route(mid, up, down) == 1:
            lo = mid
        else:
            hi = mid
    nx = 300
    for nh in (lo, lo + 1):
        assert _route(nh, up, down) == (1 if nh == lo else 0)
        x, h = _rand(27400 + up + nh, 2, nx, nh)
        _both(fft32, plain32, x, h, up, down, 0, full_len(nx, nh, up, down), f"seam {up}/{down} nh={nh}", run=_dev)


# (up, down, nx, nh, t0, out_len or None for every output from t0)
EDGES = [(3, 2, 1, 7, 0, None),     # nx == 1
         (3, 2, 50, 1, 0, None),    # nh == 1
         (1, 1, 50, 1, 0, None),    # a copy scaled by the tap
         (7, 2, 40, 3, 0, None),    # up > nh: phases 3 .. 6 have no taps
         (2, 9, 100, 3, 0, None),   # down > nh: samples no output reads
         (3, 2, 4, 31, 0, None),    # nx < nh / up: no output has all its terms
         (3, 2, 50, 31, 17, 1)]     # one output


@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("up,down,nx,nh,t0,out_len", EDGES)
def test_edges(fft32, plain32, rows, up, down, nx, nh, t0, out_len):
    if out_len is None:
        out_len = -(-((nx - 1) * up + nh - t0) // down)
    x, h = _rand(27500 + nx + nh, rows, nx, nh)
    what = f"edge up={up} down={down} rows={rows} nx={nx} nh={nh} t0={t0} out_len={out_len}"
    got = _both(fft32, plain32, x, h, up, down, t0, out_len, what)
    _both(fft32, plain32, x, h, up, down, t0, out_len, what + " dev", run=_dev)
    if up > nh:
        p = (t0 + np.arange(out_len) * down) % up
        assert (got[:, p >= nh].view(np.uint32) == 0).all(), "an output without terms is +0"


def test_windows(fft32, plain32):
    """Windows (t0, out_len) of one shape against the same slice of the full oracle (every up-sampled time: down = 1)."""
    up, down, nx, nh, rows = 3, 2, 3000, 31, 3
    x, h = _rand(27600, rows, nx, nh)
    full_up = (nx - 1) * up + nh
    every = resample_ref(x, h, up, 1, 0, full_up)
    windows = [(7, 1500),                                  # t0 mod up != 0
               ((nh - 1) // 2, -(-nx * up // down)),       # resample_poly's
               (full_up - 1 - 4 * down, 5),                # the last permitted output
               (4001, T + 76),                             # the middle of the row, two tiles
               (0, full_len(nx, nh, up, down))]
    for t0, out_len in windows:
        assert t0 + (out_len - 1) * down < full_up
        want = np.ascontiguousarray(every[:, t0::down][:, :out_len])
        assert want.shape == (rows, out_len)
        for run in (_host, _dev):
            _both(fft32, plain32, x, h, up, down, t0, out_len, f"window t0={t0} out_len={out_len} {run.__name__}", want, run=run)
    import kofft_amd

    with pytest.raises(kofft_amd.FftError) as e:  # one output further is wholly past the result
        fft32.resample_rows(x, h, up, down, full_up - 1 - 4 * down, 6)
    assert e.value.code == kofft_amd.FftError.MismatchedLengths


@pytest.mark.parametrize("nh", [4 * 4099 + 1, 2 * 4099])
def test_64_bit_positions(fft32, plain32, nh):
    """up = 4099 on 2^21 samples: up-sampled times around 2^33.  The last 300 outputs; the oracle gets the last samples and their
    offset.  4 * 4099 + 1 taps are the plain kernel's on both contexts, 2 * 4099 the tiled kernel's on the default one."""
    up, down, nx, out_len = 4099, 1, 1 << 21, 300
    assert _route(nh, up, down) == (1 if nh == 2 * 4099 else 0)
    full_up = (nx - 1) * up + nh
    assert full_up > 1 << 33
    t0 = full_up - out_len
    x, h = _rand(27700 + nh, 1, nx, nh)
    want = resample_ref(x[:, -16:], h, up, down, t0, out_len, x_first=nx - 16, nx=nx)
    assert np.count_nonzero(want) > out_len // 2
    _both(fft32, plain32, x, h, up, down, t0, out_len, f"64-bit nh={nh}", want, run=_dev)
    assert_rows_equal(_host(fft32, x, h, up, down, t0, out_len), want, f"64-bit nh={nh} host")


def test_special_values(fft32, plain32):
    """NaN, +-Inf and -0 at known places of x: they reach exactly the outputs whose term sets hold them; every other output keeps the
    clean run's bits.  Then special taps."""
    up, down, nx, nh, rows = 3, 2, 1500, 31, 3
    x, h = _rand(27800, rows, nx, nh)
    out_len = full_len(nx, nh, up, down)
    clean = _both(fft32, plain32, x, h, up, down, 0, out_len, "special: clean")
    bad = x.copy()
    bad[0, 100] = np.nan
    bad[1, 0] = np.inf
    bad[2, nx - 1] = -np.inf
    bad[0, 700:710] = -0.0
    changed = (bad.view(np.uint32) != x.view(np.uint32)).astype(F)
    touched = resample_ref(changed, np.ones(nh, F), up, down, 0, out_len) != 0  # the outputs whose term sets hold a changed sample
    assert touched.any(axis=1).all() and not touched.all(axis=1).any()
    want = resample_ref(bad, h, up, down, 0, out_len)
    for run in (_host, _dev):
        got = _both(fft32, plain32, bad, h, up, down, 0, out_len, f"special samples {run.__name__}", want, nan_safe=True, run=run)
        assert bits_equal(got[~touched], clean[~touched]), "a special value reached an output whose terms do not hold it"
        assert not np.isfinite(got[0, touched[0]][:3]).any() and np.isinf(got[1, 0])
    for tap in (np.nan, np.inf, -np.inf, -0.0):
        taps = h.copy()
        taps[nh // 2] = tap
        _both(fft32, plain32, x, taps, up, down, 0, out_len, f"special tap {tap}", nan_safe=True)
    zeros = np.full((rows, nx), -0.0, F)
    got = _both(fft32, plain32, zeros, h, up, down, 0, out_len, "-0 samples")
    assert (got.view(np.uint32) == 0).all(), "-0 samples give +0 outputs"


@pytest.mark.parametrize("up,down,nh", [(3, 2, 31), (160, 441, 1765), (3, 2, 20001)])
def test_unaligned_device_buffers(fft32, plain32, up, down, nh):
    """Device buffers that are only 4-byte aligned (views one float into their allocations), on both routes."""
    nx = 2500
    x, h = _rand(27900 + nh, 3, nx, nh)
    _both(fft32, plain32, x, h, up, down, 0, full_len(nx, nh, up, down), f"unaligned {up}/{down} nh={nh}", run=_dev, off=1)


@pytest.mark.parametrize("rows,nx", [(8, 10000), (8, 200000)])
def test_host_equals_device(fft32, plain32, rows, nx):
    """The host entry and the device entry give the same bytes: 320 KB in (zero-copy) and 6.4 MB (staged), 48 -> 16 kHz."""
    up, down, nh = 1, 3, 61
    x, h = _rand(28000 + nx, rows, nx, nh)
    t0, out_len = (nh - 1) // 2, -(-nx // 3)
    want = resample_ref(x, h, up, down, t0, out_len)
    for f in (fft32, plain32):
        got = _host(f, x, h, up, down, t0, out_len)
        assert_rows_equal(got, want, f"host rows={rows} nx={nx}")
        assert bits_equal(got, _dev(f, x, h, up, down, t0, out_len)), f"host against device rows={rows} nx={nx}"


@pytest.mark.parametrize("up,down", [(160, 441), (1, 3)])
def test_module_resample_poly(fft32, plain32, up, down):
    """kofft_amd.resample.resample_poly on [2, 4410]: the oracle with the helper's taps bit for bit, scipy in float64 under the CPU
    bound (tests/test_resample_cpu.py), the gcd reduction."""
    from scipy import signal

    from kofft_amd import resample

    x = seeded(28100 + up).uniform(-1, 1, (2, 4410)).astype(F)
    taps = resample.design_taps(up, down)
    nh, out_len = taps.size, -(-4410 * up // down)
    t0 = (nh - 1) // 2
    want = resample_ref(x, taps, up, down, t0, out_len)
    want64 = signal.resample_poly(x.astype(np.float64), up, down, axis=1)
    assert want64.shape == (2, out_len)
    for f in (fft32, plain32):
        got = resample.resample_poly(x, up, down, fft=f)
        assert_rows_equal(got, want, f"resample_poly {up}/{down}")
        assert bits_equal(got, resample.resample_poly(x, 2 * up, 2 * down, fft=f)), "the gcd is not reduced"
        assert bits_equal(got, resample.resample_poly(x, up, down, taps=taps, fft=f))
        for r in range(2):
            bound = forward_bound(x[r], taps, up, down, t0, out_len)
            err = np.abs(got[r].astype(np.float64) - want64[r])
            print(f"{up}/{down} row {r}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
            assert (err <= bound).all(), (r, int(np.argmax(err - bound)))
    one = resample.resample_poly(x[0], up, down, fft=fft32)
    assert one.shape == (out_len,) and bits_equal(one, want[0])


def test_module_upfirdn_copy_and_short_taps(fft32, plain32):
    from kofft_amd import resample

    x, h = _rand(28200, 4, 1000, 33)
    for up, down in [(1, 1), (3, 2), (2, 5)]:
        want = resample_ref(x, h, up, down, 0, full_len(1000, 33, up, down))
        for f in (fft32, plain32):
            assert_rows_equal(resample.upfirdn(h, x, up, down, fft=f), want, f"upfirdn {up}/{down}")
        assert bits_equal(resample.upfirdn(h, x[0], up, down, fft=fft32), want[0])
    got = resample.resample_poly(x, 7, 7, fft=fft32)
    assert bits_equal(got, x) and not np.shares_memory(got, x)
    # taps so short that the last outputs of resample_poly lie past the full result: +0 there, as scipy pads
    short = np.array([0.5, 1.0, 0.5], F)
    got = resample.resample_poly(x, 8, 1, taps=short, fft=fft32)
    assert got.shape == (4, 8000)
    full_up = 999 * 8 + 3
    assert_rows_equal(got[:, :full_up - 1], resample_ref(x, short, 8, 1, 1, full_up - 1), "short taps")
    assert (got[:, full_up - 1:].view(np.uint32) == 0).all()


def test_errors_that_need_a_context(fft32):
    import torch

    import kofft_amd

    E = kofft_amd.FftError
    x = np.ones((2, 10), F)
    h = np.ones(5, F)
    for kw, code in [(dict(up=0), E.InvalidValue), (dict(down=0), E.InvalidValue), (dict(t0=14, out_len=1), E.MismatchedLengths),
                     (dict(up=2, t0=0, out_len=25), E.MismatchedLengths)]:
        with pytest.raises(E) as e:
            fft32.resample_rows(x, h, **kw)
        assert e.value == E(code), kw
    with pytest.raises(E) as e:
        fft32.resample_rows(x, np.ones(0, F))
    assert e.value == E(E.EmptyInput)
    assert fft32.resample_rows(x, h, out_len=0).shape == (2, 0)
    assert fft32.resample_rows(np.ones((0, 10), F), h).shape == (0, 14)
    assert fft32.resample_rows(x, h, 2, 1).shape == (2, 23)
    buf = torch.zeros(256, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    with pytest.raises(kofft_amd.DeviceError):
        fft32.resample_dev(0, 2, 10, p + 400, 5, 1, 1, 0, p + 512, 14)  # a null signal
    for d_x, d_h, d_out in [(p, p + 400, p + 36), (p, p + 400, p + 300), (p + 512, p, p + 16)]:
        with pytest.raises(E) as e:
            fft32.resample_dev(d_x, 2, 10, d_h, 5, 1, 1, 0, d_out, 14)  # the output over the signal / over the taps
        assert e.value == E(E.InvalidValue), (d_x - p, d_h - p, d_out - p)
    fft32.synchronize()
    assert not buf.any()  # nothing ran
