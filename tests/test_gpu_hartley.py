"""hartley::dht on the device, bit for bit against tests/hartley_oracle.py (NaNs by position: the host and the device produce
different default NaNs).  The table the device builds (dht_table_kernel, the restated sinf / cosf on the device's f64 path) is read
back entry by entry through rows of unit vectors; random rows check the sums on both kernels of the direct family, with the table built
on the device and on the host; every device-pointer call of this module runs inside the guard bands of tests/redzone.py.

Shapes: the tiled kernel's tile is 128 rows x 128 columns, the tiled / simple crossover at n = 64 and batch = 64; the table kernel's
lane owns four columns and its workgroup 1024 of them, the table's row stride is n rounded up to 128."""
import ctypes as C

import numpy as np
import pytest

import hartley_oracle as ho
from conftest import bits_equal, seeded
from redzone import Arena
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32

TABLE_NS = [1, 2, 3, 5, 64, 127, 128, 129, 1000, 4096]
NS = [1, 2, 3, 4, 7, 63, 64, 65, 128, 255, 256, 1000]
BATCHES = [1, 63, 64, 65, 129, 257]


@pytest.fixture(scope="module")
def simple32():
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_direct_tiled(False)
    yield f
    f.close()


@pytest.fixture(scope="module")
def hosttab32():
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_dht_table_device(False)
    yield f
    f.close()


def _run(f, x):
    a = f.dht_batch(x)
    b = f.dht_batch(x)
    assert bits_equal(a, b), "two runs of the same call differ"
    return a


def _lib_table(f, n):
    h = np.empty((n, n), F)
    assert f._lib.kofft_hip_dht_table_f32(n, C.c_void_p(h.ctypes.data)) == 0
    return h


@pytest.mark.parametrize("n", TABLE_NS)
def test_unit_vectors_read_the_device_table_back(n):
    """out[i][k] = H[i][k] exactly (the other terms are +-0 onto a +0 seed): every entry the device's f64 path produced equals the
    host's table, whose restatement tests/test_hartley_cpu.py holds against the oracle on every angle of these lengths."""
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)  # a fresh context: its table of this length is built by dht_table_kernel in this call
    try:
        got = f.dht_batch(np.eye(n, dtype=F))
        want = _lib_table(f, n)
        assert_rows_equal(got, want, f"device table n={n}")
        if n <= 1000:
            assert_rows_equal(got, ho.table(n), f"device table against the oracle n={n}")
        f.set_direct_tiled(False)
        assert bits_equal(f.dht_batch(np.eye(n, dtype=F)[: min(n, 130)]), want[: min(n, 130)]), "the simple kernel reads the same table"
    finally:
        f.close()


def _rows(n, batch, seed):
    """Random rows; row 1 all -0, row 2 with inf and NaN planted (where the batch has them)."""
    x = seeded(seed).uniform(-1, 1, (batch, n)).astype(F)
    if batch > 1:
        x[1] = -0.0
    if batch > 2:
        x[2, 0] = np.inf
        x[2, n // 2] = np.nan
        x[2, n - 1] = -np.inf
    return x


@pytest.mark.parametrize("n", NS)
def test_random_rows_every_route(fft32, simple32, hosttab32, n):
    x_all = _rows(n, max(BATCHES), 21000 + n)
    want_all = ho.dht(x_all)  # once per length: a row's result does not depend on the batch
    for batch in BATCHES:
        x = np.ascontiguousarray(x_all[:batch])
        what = f"n={n} batch={batch}"
        got = _run(fft32, x)
        assert_rows_equal(got, want_all[:batch], what, nan_safe=True)
        assert_rows_equal(_run(simple32, x), got, what + ": set_direct_tiled(0)", nan_safe=True)
        assert_rows_equal(_run(hosttab32, x), got, what + ": set_dht_table_device(0)", nan_safe=True)
        if batch > 1:
            assert bits_equal(got[1], np.zeros(n, F)), "a row of -0 gives +0 (the +0 seed)"
        if batch > 2 and n >= 2:
            assert np.isnan(got[2]).any(), "inf and NaN inputs reach the outputs"


def test_full_size(fft32, simple32, hosttab32):
    """n = 4096 once, at batch 130: every row, on both ends, both sides of every 128-column tile edge and seeded other columns against
    the oracle; every column between the routes."""
    n, batch = 4096, 130
    x = _rows(n, batch, 22000)
    cols = ho.sample_cols(n, 96, 22001)
    got = _run(fft32, x)
    assert_rows_equal(np.ascontiguousarray(got[:, cols]), ho.dht(x, cols=cols), "n=4096 batch=130", nan_safe=True)
    assert_rows_equal(_run(simple32, x), got, "n=4096: set_direct_tiled(0)", nan_safe=True)
    assert_rows_equal(_run(hosttab32, x), got, "n=4096: set_dht_table_device(0)", nan_safe=True)
    assert bits_equal(got[1], np.zeros(n, F))


def test_the_references_own_pins(fft32):
    """hartley.rs:63-70, 90-125."""
    from kofft_amd import hartley

    x = np.array([1.0, 2.0, 3.0, 4.0], F)
    z = hartley.dht(hartley.dht(x, fft=fft32), fft=fft32)
    assert np.all(np.abs(x - z / F(4.0)) < 1e-5), z
    assert bits_equal(hartley.dht(np.zeros(8, F), fft=fft32), np.zeros(8, F))
    assert np.any(np.abs(hartley.dht(np.ones(8, F), fft=fft32)) > 0)
    assert hartley.dht(np.zeros(0, F), fft=fft32).shape == (0,)
    one = hartley.dht(np.array([1.0], F), fft=fft32)
    assert one.shape == (1,) and one[0] == 1.0


def _dev(f, d_in, d_out, n, batch):
    p_in, p_out = (None if p is None else C.c_void_p(int(p)) for p in (d_in, d_out))
    return f._lib.kofft_hip_dev_dht_f32(f._ctx, p_in, p_out, n, batch)


def test_host_form_in_place_and_argument_edges(fft32):
    import torch

    x = _rows(129, 70, 23000)
    want = ho.dht(x)
    buf = x.copy()
    fft32._check(fft32._lib.kofft_hip_dht_f32(fft32._ctx, buf.ctypes.data, buf.ctypes.data, 129, 70))  # in == out
    assert_rows_equal(buf, want, "host form, in == out", nan_safe=True)
    d = torch.zeros(4 * 64, device="cuda")
    assert _dev(fft32, d.data_ptr(), d.data_ptr() + 4 * 8, 64, 3) == 6  # overlapping device buffers: INVALID_VALUE
    assert _dev(fft32, d.data_ptr(), d.data_ptr(), 64, 3) == 6
    assert _dev(fft32, d.data_ptr(), d.data_ptr() + 4 * 128, 64, 2) == 0  # adjacent is not overlap
    torch.cuda.synchronize()
    assert _dev(fft32, d.data_ptr(), d.data_ptr(), 4097, 1) == -2
    assert fft32._lib.kofft_hip_dht_f32(fft32._ctx, buf.ctypes.data, buf.ctypes.data, 4097, 1) == -2
    assert _dev(fft32, None, None, 0, 5) == 0 and fft32._lib.kofft_hip_dht_f32(fft32._ctx, None, None, 0, 5) == 0  # n == 0
    assert _dev(fft32, None, None, 8, 0) == 0
    assert _dev(fft32, None, d.data_ptr(), 8, 1) == -3


# (n, batch, align_off of the output in bytes): both kernels, a ragged last row tile, 4-byte aligned outputs (no 16-byte stores)
GUARD_CASES = [(5, 3, 0), (64, 64, 0), (65, 129, 0), (128, 130, 4), (1000, 65, 0), (255, 257, 12)]


@pytest.mark.parametrize("n,batch,off", GUARD_CASES)
def test_guard_bands_device_form(fft32, n, batch, off):
    x = _rows(n, batch, 24000 + n)
    arena = Arena("cuda", f"dev_dht n={n} batch={batch} off={off}")
    d_in = arena.input(x, row_bytes=4 * n)
    d_out = arena.output(4 * n * batch, align_off=off, row_bytes=4 * n)
    for _ in range(2):
        assert _dev(fft32, d_in.addr, d_out.addr, n, batch) == 0
    arena.verify()
    assert_rows_equal(arena.read(d_out, F, (batch, n)), ho.dht(x), arena.what, nan_safe=True)


@pytest.mark.parametrize("n,batch,off", GUARD_CASES[:4])
def test_guard_bands_host_form(fft32, n, batch, off):
    x = _rows(n, batch, 24500 + n)
    arena = Arena("host", f"dht n={n} batch={batch} off={off}")
    h_in = arena.input(x, row_bytes=4 * n)
    h_out = arena.output(4 * n * batch, align_off=off, row_bytes=4 * n)
    fft32._check(fft32._lib.kofft_hip_dht_f32(fft32._ctx, C.c_void_p(h_in.addr), C.c_void_p(h_out.addr), n, batch))
    arena.verify()
    assert_rows_equal(arena.read(h_out, F, (batch, n)), ho.dht(x), arena.what, nan_safe=True)


def test_context_lifecycle_and_streams():
    """Two lengths alternately on one context, a second context, kofft_hip_release_scratch between calls, and the cached table used
    from another stream (kofft_hip_set_stream orders the new stream after the table's kernel)."""
    import torch

    import kofft_amd

    xa, xb = _rows(65, 70, 25000), _rows(200, 66, 25001)
    wa, wb = ho.dht(xa), ho.dht(xb)
    c1, c2 = kofft_amd.HipFftImpl(F), kofft_amd.HipFftImpl(F)
    try:
        for _ in range(2):
            assert_rows_equal(c1.dht_batch(xa), wa, "c1 n=65", nan_safe=True)
            assert_rows_equal(c1.dht_batch(xb), wb, "c1 n=200", nan_safe=True)
        assert_rows_equal(c2.dht_batch(xb), wb, "c2 n=200", nan_safe=True)
        c1.release_scratch()
        assert_rows_equal(c1.dht_batch(xa), wa, "c1 after release_scratch", nan_safe=True)
        # device form: the table of n = 200 was built on the context's own stream, the table of n = 33 is built on s
        s = torch.cuda.Stream()
        xc = _rows(33, 5, 25002)
        d_b, d_c = torch.from_numpy(xb).cuda(), torch.from_numpy(xc).cuda()
        o_b, o_c = torch.empty_like(d_b), torch.empty_like(d_c)
        torch.cuda.synchronize()
        c1.set_stream(s.cuda_stream)
        c1.dht_dev(d_b.data_ptr(), o_b.data_ptr(), 200, 66)
        c1.dht_dev(d_c.data_ptr(), o_c.data_ptr(), 33, 5)
        c1.synchronize()
        c1.set_stream(0)
        assert_rows_equal(o_b.cpu().numpy(), wb, "cached table on another stream", nan_safe=True)
        assert_rows_equal(o_c.cpu().numpy(), ho.dht(xc), "table built on another stream", nan_safe=True)
        assert_rows_equal(c1.dht_batch(xc), ho.dht(xc), "back on the own stream", nan_safe=True)
    finally:
        c1.close()
        c2.close()


def test_python_module_on_ragged_lists(fft32):
    from kofft_amd import hartley

    rng = seeded(26000)
    x2 = rng.uniform(-1, 1, (3, 40)).astype(F)
    assert bits_equal(hartley.dht(x2, fft=fft32), ho.dht(x2))
    x1 = rng.uniform(-1, 1, 40).astype(F)
    assert bits_equal(hartley.dht(x1), ho.dht(x1[None])[0])  # the module's own context
    for fn in (hartley.batch, hartley.multi_channel):
        rows = [rng.uniform(-1, 1, m).astype(F) for m in (5, 64, 5, 1, 300, 64, 0)]
        want = [ho.dht(r[None])[0] for r in rows]
        fn(rows, fft=fft32)
        for r, w in zip(rows, want):
            assert bits_equal(r, w)
