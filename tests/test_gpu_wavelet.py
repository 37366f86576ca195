"""The wavelet transforms on the device against tests/wavelet_oracle.py, every row bit for bit: single level (the streaming kernels),
multi level on the fused kernels and level by level, the host, _dev and module forms."""
import os

import numpy as np
import pytest

import wavelet_oracle as wo
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu

F = np.float32
FUSED_MAX = 16384  # include/kofft_hip.h: the longest row the fused multi-level kernels take
LENGTHS = [1, 2, 3, 5, 7, 8, 9, 16, 17, 31, 100, 1000, 1024, 4097, 16384, FUSED_MAX + 1, 65536, 1 << 20]


def _batch(n):
    return max(1, min(37, (1 << 21) // max(n, 1)))


def _x(shape, seed):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(F)


@pytest.fixture(scope="module")
def fused():
    """The fused multi-level kernels wherever the row fits (set_wavelet_fused(2)), so every instance runs."""
    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    f.set_wavelet_fused(2)
    return f


@pytest.fixture(scope="module")
def auto():
    """The default route: the fused kernels only where they measured faster."""
    import kofft_amd

    return kofft_amd.HipFftImpl(np.float32)


@pytest.fixture(scope="module")
def perlevel():
    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    f.set_wavelet_fused(False)
    return f


def _levels(n):
    deep = 0
    while (n >> deep) > 1 and deep < 40:
        deep += 1
    if (1 << deep) < n:
        deep += 1
    return sorted({0, 1, 3, deep, deep + 3})


@pytest.mark.parametrize("name", wo.NAMES)
@pytest.mark.parametrize("n", LENGTHS)
def test_single_level(fused, name, n):
    """<name>_forward on rows of n, <name>_inverse on rows of max(1, n // 2), every row against the oracle."""
    b = _batch(n)
    x = _x((b, n), 1000 + n)
    a, d = fused.dwt_batch(x, name)
    wa, wd = wo.forward(name, x)
    assert_rows_equal(a, wa, f"{name} forward n={n} approx")
    assert_rows_equal(d, wd, f"{name} forward n={n} detail")
    h = max(1, n // 2)
    ia, idt = _x((b, h), 2000 + n), _x((b, h), 3000 + n)
    y = fused.idwt_batch(ia, idt, name)
    assert_rows_equal(y, wo.inverse(name, ia, idt), f"{name} inverse n={h}")
    assert fused.idwt_batch(ia, idt, name).tobytes() == y.tobytes(), "two runs differ"


@pytest.mark.parametrize("name", wo.NAMES)
@pytest.mark.parametrize("n", LENGTHS)
def test_multi_level_fused_and_per_level(fused, perlevel, auto, name, n):
    """multi_level_forward / _inverse at levels {0, 1, 3, the level where the length reaches 1, 3 past it}: the fused and the
    per-level route (and the default choice between them) give the oracle's bytes."""
    b = max(1, min(9, (1 << 20) // n))
    x = _x((b, n), 4000 + n)
    for levels in _levels(n):
        wa, wds = wo.forward_multi(name, x, levels)
        for f, route in ((fused, "fused"), (perlevel, "per-level"), (auto, "default")):
            a, ds = f.wavedec_batch(x, name, levels)
            assert_rows_equal(a, wa, f"{name} n={n} L={levels} {route} approx")
            assert len(ds) == levels
            for l, (g, w) in enumerate(zip(ds, wds)):
                assert_rows_equal(g, w, f"{name} n={n} L={levels} {route} detail {l}")
        # the inverse from rows that fold without a mismatch: n0 approximations, detail l holds n0 << (levels - 1 - l) (+1: ignored)
        n0 = max(1, n >> levels) if levels else n
        if n0 << levels > (1 << 20):
            continue
        ap = _x((b, n0), 5000 + n + levels)
        dets = [_x((b, (n0 << (levels - 1 - l)) + (l % 2)), 6000 + 7 * l + n) for l in range(levels)]
        want = wo.inverse_multi(name, ap, dets)
        for f, route in ((fused, "fused"), (perlevel, "per-level"), (auto, "default")):
            assert_rows_equal(f.waverec_batch(ap, dets, name), want, f"{name} inverse n0={n0} L={levels} {route}")


@pytest.mark.parametrize("name", ["haar", "db2", "coif1", "sym4"])
@pytest.mark.parametrize("n,batches", [(8, [1, 2, 1023, 1024, 1025, 3001]), (100, [1, 19, 20, 21, 81, 82, 83]),
                                       (1000, [1, 7, 8, 9, 17]), (1026, [3, 5]), (3000, [1, 2, 3, 5])])
def test_batch_ladders(fused, perlevel, name, n, batches):
    """Batches around the rows per workgroup of the streaming kernels (1024 / n outputs) and of the fused kernels (8192 / n)."""
    for b in batches:
        x = _x((b, n), 7000 + b + n)
        a, d = fused.dwt_batch(x, name)
        wa, wd = wo.forward(name, x)
        assert_rows_equal(a, wa, f"{name} n={n} b={b}")
        assert_rows_equal(d, wd, f"{name} n={n} b={b}")
        wa, wds = wo.forward_multi(name, x, 3)
        for f in (fused, perlevel):
            a, ds = f.wavedec_batch(x, name, 3)
            assert_rows_equal(a, wa, f"{name} multi n={n} b={b}")
            for g, w in zip(ds, wds):
                assert_rows_equal(g, w, f"{name} multi detail n={n} b={b}")
        m = n // 8
        ap = _x((b, m), 7100 + b)
        dets = [_x((b, m << (2 - l)), 7200 + l + b) for l in range(3)]
        want = wo.inverse_multi(name, ap, dets)
        for f in (fused, perlevel):
            assert_rows_equal(f.waverec_batch(ap, dets, name), want, f"{name} inverse multi n={n} b={b}")
        y = fused.idwt_batch(ap, dets[2][:, :m], name)
        assert_rows_equal(y, wo.inverse(name, ap, dets[2][:, :m]), f"{name} inverse n={m} b={b}")


def test_grid_stride_over_row_groups(fused):
    """More row groups than the grid's 65535 rows (the streaming kernels stride over them)."""
    n, b = 1026, 65537
    x = _x((b, n), 8100)
    a, d = fused.dwt_batch(x, "haar")
    wa, wd = wo.forward("haar", x)
    assert_rows_equal(a, wa, "haar grid-stride approx")
    assert_rows_equal(d, wd, "haar grid-stride detail")


def _special_rows(n, rng):
    specials = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1.2e-38, np.inf, -np.inf, np.nan, 3e38, -3e38], F)
    rows = [np.full(n, v, F) for v in (-0.0, 0.0, 1e-40, -1e-45, 3e38, np.inf)]
    for j in range(len(specials)):
        r = rng.uniform(-1, 1, n).astype(F)
        r[rng.choice(n, size=min(n, 1 + j % 3), replace=False)] = specials[j]
        rows.append(r)
    rows.append(specials[rng.integers(0, len(specials), n)])
    return np.stack(rows)


@pytest.mark.parametrize("name", wo.NAMES)
@pytest.mark.parametrize("n", [2, 5, 8, 17, 64, 1000, 4097])
def test_special_values(fused, perlevel, name, n):
    """+-0 (db2 keeps -0, the seeded sums give +0), subnormals, +-Inf, NaN and overflow, through every kernel."""
    x = _special_rows(n, np.random.default_rng(8200 + n))
    with np.errstate(all="ignore"):
        wa, wd = wo.forward(name, x)
        a, d = fused.dwt_batch(x, name)
        assert_rows_equal(a, wa, f"{name} n={n}", nan_safe=True)
        assert_rows_equal(d, wd, f"{name} n={n}", nan_safe=True)
        h = max(1, n // 2)
        y = fused.idwt_batch(np.ascontiguousarray(x[:, :h]), np.ascontiguousarray(x[:, -h:]), name)
        assert_rows_equal(y, wo.inverse(name, x[:, :h], x[:, -h:]), f"{name} inverse n={h}", nan_safe=True)
        wa, wds = wo.forward_multi(name, x, 2)
        for f in (fused, perlevel):
            a, ds = f.wavedec_batch(x, name, 2)
            assert_rows_equal(a, wa, f"{name} multi n={n}", nan_safe=True)
            for g, w in zip(ds, wds):
                assert_rows_equal(g, w, f"{name} multi n={n}", nan_safe=True)
        if n % 4 == 0:
            q = n // 4
            dets = [np.ascontiguousarray(x[:, :2 * q]), np.ascontiguousarray(x[:, -q:])]
            ap = np.ascontiguousarray(x[:, q:2 * q])
            want = wo.inverse_multi(name, ap, dets)
            for f in (fused, perlevel):
                assert_rows_equal(f.waverec_batch(ap, dets, name), want, f"{name} inverse multi n={n}", nan_safe=True)


@pytest.mark.parametrize("name", ["db2", "db4", "coif1"])
def test_host_form_equals_dev_form_offsets_and_overlap(fused, name):
    """The host forms (zero-copy below 512 KiB, staged above) give the _dev forms' bytes, also with every pointer 4 bytes off a
    16-byte boundary; an output overlapping an input is refused."""
    import torch

    import kofft_amd

    for n, b, levels in ((1000, 4, 3), (16384, 64, 5), (4097, 40, 2), (65536, 9, 4)):
        x = _x((b, n), 9000 + n)
        a, d = fused.dwt_batch(x, name)
        wa, wds = fused.wavedec_batch(x, name, levels)
        lens = kofft_amd.api.dwt_multi_lengths(n, levels)
        for off in (0, 1):
            dx = torch.zeros(b * n + off, dtype=torch.float32, device="cuda")
            dx[off:] = torch.from_numpy(x.ravel()).cuda()
            da = torch.full((b * (n // 2) + off,), 7.0, device="cuda")
            dd = torch.full((b * (n // 2) + off,), 7.0, device="cuda")
            fused.dwt_dev(name, dx.data_ptr() + 4 * off, da.data_ptr() + 4 * off, dd.data_ptr() + 4 * off, n, b)
            fused.synchronize()
            assert da[off:].cpu().numpy().tobytes() == a.tobytes() and dd[off:].cpu().numpy().tobytes() == d.tobytes()
            dy = torch.zeros(b * 2 * (n // 2) + off, device="cuda")
            fused.idwt_dev(name, da.data_ptr() + 4 * off, dd.data_ptr() + 4 * off, dy.data_ptr() + 4 * off, n // 2, b)
            fused.synchronize()
            assert dy[off:].cpu().numpy().tobytes() == fused.idwt_batch(a, d, name).tobytes()
            tot = sum(lens[1:])
            dap = torch.zeros(b * lens[-1] + off, device="cuda")
            ddet = torch.zeros(b * tot + off, device="cuda")
            fused.wavedec_dev(name, dx.data_ptr() + 4 * off, dap.data_ptr() + 4 * off, ddet.data_ptr() + 4 * off, n, b, levels)
            fused.synchronize()
            assert dap[off:].cpu().numpy().tobytes() == wa.tobytes()
            assert ddet[off:].cpu().numpy().tobytes() == np.concatenate([w.ravel() for w in wds]).tobytes()
            if all(m % 2 == 0 for m in lens[1:levels]):
                dout = torch.zeros(b * (lens[-1] << levels) + off, device="cuda")
                fused.waverec_dev(name, dap.data_ptr() + 4 * off, ddet.data_ptr() + 4 * off, lens[1:], dout.data_ptr() + 4 * off,
                                  lens[-1], b)
                fused.synchronize()
                assert dout[off:].cpu().numpy().tobytes() == fused.waverec_batch(wa, wds, name).tobytes()
    buf = torch.zeros(4096, device="cuda")
    with pytest.raises(kofft_amd.FftError):
        fused.dwt_dev(name, buf.data_ptr(), buf.data_ptr() + 4 * 100, buf.data_ptr() + 4 * 2000, 512, 2)
    with pytest.raises(kofft_amd.FftError):
        fused.wavedec_dev(name, buf.data_ptr(), buf.data_ptr() + 4 * 3000, buf.data_ptr() + 4 * 100, 512, 2, 2)


def test_host_pipeline(monkeypatch):
    """Single-level host calls of 128 MiB and more through the chunked pipeline give the oracle's bytes."""
    import kofft_amd

    monkeypatch.setenv("KOFFT_HIP_HOST_PIPELINE", "1")
    f = kofft_amd.HipFftImpl(np.float32)
    n, b = 1 << 20, 20
    x = _x((b, n), 9500)
    a, d = f.dwt_batch(x, "sym4")
    wa, wd = wo.forward("sym4", x)
    assert_rows_equal(a, wa, "pipelined forward")
    assert_rows_equal(d, wd, "pipelined forward")
    y = f.idwt_batch(a, d, "sym4")
    assert_rows_equal(y, wo.inverse("sym4", a, d), "pipelined inverse")
    f.close()


def test_route_switch_values(auto):
    """set_wavelet_fused takes 0, 1, 2 (False / True) and nothing else."""
    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    for mode in (0, 2, 1, False, True):
        f.set_wavelet_fused(mode)
    with pytest.raises(ValueError):
        f.set_wavelet_fused(3)
    assert f._lib.kofft_hip_set_wavelet_fused(f._ctx, 3) == 6
    f.close()


def test_module_functions(fused):
    """kofft_amd.wavelet: the reference's names, ragged batches (one call per length), foreign callables, the reference's tests."""
    from kofft_amd import wavelet as wv

    rng = np.random.default_rng(9700)
    rows = [rng.uniform(-1, 1, n).astype(F) for n in (8, 13, 8, 1, 0, 100, 13, 4097)]
    for name in wo.NAMES:
        fwd, inv = getattr(wv, f"{name}_forward"), getattr(wv, f"{name}_inverse")
        for r in rows:
            a, d = fwd(r, fused)
            wa, wd = wo.forward(name, r.reshape(1, -1))
            assert a.tobytes() == wa.tobytes() and d.tobytes() == wd.tobytes()
            if a.size:
                assert inv(a, d, fused).tobytes() == wo.inverse(name, wa, wd).tobytes()
            for levels in (0, 2, 5):
                ma, mds = getattr(wv, f"{name}_forward_multi")(r, levels, fused)
                ra, rds = wo.forward_multi(name, r.reshape(1, -1), levels)
                assert ma.tobytes() == ra.tobytes() and [m.tobytes() for m in mds] == [m.tobytes() for m in rds]
        if name in ("haar", "db2"):
            bf, bi = (wv.batch_forward, wv.batch_inverse) if name == "haar" else (wv.db2_forward_batch, wv.db2_inverse_batch)
            avgs, diffs = bf(rows, fused)
            for r, a, d in zip(rows, avgs, diffs):
                wa, wd = wo.forward(name, r.reshape(1, -1))
                assert a.tobytes() == wa.tobytes() and d.tobytes() == wd.tobytes()
            rec = bi(avgs, diffs, fused)
            for a, d, y in zip(avgs, diffs, rec):
                assert y.tobytes() == wo.inverse(name, a.reshape(1, -1), d.reshape(1, -1)).tobytes()
        avgs, dets = wv.multi_level_forward_batch(rows, 2, fwd, fused)
        for r, a, ds in zip(rows, avgs, dets):
            ra, rds = wo.forward_multi(name, r.reshape(1, -1), 2)
            assert a.tobytes() == ra.tobytes() and [m.tobytes() for m in ds] == [m.tobytes() for m in rds]
        ok = [j for j, r in enumerate(rows) if all(m % 2 == 0 for m in wo.multi_lengths(r.size, 2)[1:2]) or r.size == 0]
        rec = wv.multi_level_inverse_batch([avgs[j] for j in ok], [dets[j] for j in ok], inv, fused)
        for j, y in zip(ok, rec):
            assert y.tobytes() == wo.inverse_multi(name, avgs[j].reshape(1, -1), [m.reshape(1, -1) for m in dets[j]]).tobytes()
    # a foreign callable runs the reference's loop around it; the module's own functions as foreign-looking lambdas agree
    x = rng.uniform(-1, 1, 37).astype(F)
    a1, d1 = wv.multi_level_forward(x, 4, lambda s: wv.db4_forward(s, fused))
    a2, d2 = wv.multi_level_forward(x, 4, wv.db4_forward, fused)
    assert a1.tobytes() == a2.tobytes() and [m.tobytes() for m in d1] == [m.tobytes() for m in d2]
    y1 = wv.multi_level_inverse(a2[:2], [m[:16] for m in d2[:2]] + [], lambda a, d: wv.db4_inverse(a, d, fused))
    y2 = wv.multi_level_inverse(a2[:2], [m[:16] for m in d2[:2]], wv.db4_inverse, fused)
    assert y1.tobytes() == y2.tobytes()
    # wavelet.rs's own tests
    xs = [np.array([1, 2, 3, 4, 5, 6, 7, 8], F), np.array([5, 6, 7, 8, 1, 2, 3, 4], F)]
    avgs, diffs = wv.batch_forward(xs, fused)
    for o, r in zip(xs, wv.batch_inverse(avgs, diffs, fused)):
        assert np.all(np.abs(o - r) < 1e-6)
    sa, sd = wv.sym4_forward_multi(xs[0], 2, fused)
    assert wv.sym4_inverse_multi(sa, sd, fused).shape == (8,)
    ca, cd = wv.coif1_forward_multi(xs[0], 2, fused)
    assert wv.coif1_inverse_multi(ca, cd, fused).shape == (8,)
