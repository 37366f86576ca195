"""czt::czt_f32 and goertzel::goertzel_f32 on the device, every row bit for bit against tests/spectral_oracle.py (NaNs by position: the
host and the device produce different default NaNs), through the C ABI: host pointers, device pointers (aligned and offset by one
float), a non-default stream, all three chirp-Z routes, every call twice.  Every device-pointer call of this module runs inside the
guard bands of tests/redzone.py; the dedicated guard-band cases at the end cover the four entry points that take data pointers, and a
CPU-side assertion holds this module's case table against the header.

Shapes.  Chirp-Z: the tiled kernel's tile is 128 rows x 128 columns = 64 bins, its chunk 16 samples, the tiled / simple crossover at
nk = 2 m = 64 columns and batch = 64; lengths and bin counts sit on both sides of each and are paired so that n > m and n < m both
occur.  Goertzel: the staged chunk is 32 samples, a workgroup owns 256 // nfreq rows (nfreq < 256)."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import spectral_oracle as so
from conftest import bits_equal, seeded
from redzone import Arena
from rowcheck import assert_rows_equal

ROOT = Path(__file__).resolve().parent.parent
gpu = pytest.mark.gpu

CZT_NS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 100, 257, 1024]
CZT_MS = [1, 2, 3, 31, 32, 33, 63, 64, 65, 100, 129, 300]
CZT_BATCHES = [1, 2, 63, 64, 65, 129, 300]
GENERAL = ("dft", "zoom", "a_zero")


def _czt_cases():
    """A pruned product: every n against three bin counts (one smaller, one close, one larger where they exist), the batches cycling so
    that each appears with short and long rows; 36 cases."""
    cases = []
    for j, n in enumerate(CZT_NS):
        for t, shift in enumerate((0, 5, 9)):
            m = CZT_MS[(j + shift) % len(CZT_MS)]
            batch = CZT_BATCHES[(2 * j + 3 * t) % len(CZT_BATCHES)]
            cases.append((n, m, batch, GENERAL[(j + t) % 3]))
    return cases


class Ctx:
    """A context of the C ABI on device 0."""

    def __init__(self, lib):
        self.lib, self.h = lib, C.c_void_p()
        assert lib.kofft_hip_create(0, C.byref(self.h)) == 0

    def route(self, mode):
        assert self.lib.kofft_hip_set_czt_route(self.h, mode) == 0

    def close(self):
        if self.h:
            assert self.lib.kofft_hip_destroy(self.h) == 0
            self.h = C.c_void_p()


@pytest.fixture(scope="module")
def ctx(hiplib):
    c = Ctx(hiplib)
    yield c
    c.close()


def _ok(c, rc):
    assert rc == 0, (rc, c.lib.kofft_hip_last_error(c.h))


def czt_call(c, x, m, w, a, form="dev", runs=2):
    """kofft_hip_czt_f32 (form "host") or kofft_hip_dev_czt_f32 ("dev", "dev_off": every buffer one float past a 256-byte boundary) inside
    guard bands, `runs` times: the runs must agree, the bands and the input must be intact.  [batch, m] complex64."""
    batch, n = x.shape
    (wr, wi), (ar, ai) = so._pair(w), so._pair(a)
    arena = Arena("host" if form == "host" else "cuda", f"czt {form} n={n} m={m} batch={batch}")
    off = 4 if form == "dev_off" else 0
    xin = arena.input(x, align_off=off, row_bytes=4 * n)
    out = arena.output(8 * m * batch, align_off=off, row_bytes=8 * m)
    fn = c.lib.kofft_hip_czt_f32 if form == "host" else c.lib.kofft_hip_dev_czt_f32
    got = []
    for _ in range(runs):
        _ok(c, fn(c.h, C.c_void_p(xin.addr), C.c_void_p(out.addr), n, m, wr, wi, ar, ai, batch))
        _ok(c, c.lib.kofft_hip_synchronize(c.h))
        arena.verify()
        got.append(arena.read(out, np.complex64, (batch, m)))
        arena.restore(out)
    for g in got[1:]:
        assert bits_equal(got[0], g), f"{arena.what}: two runs of the same call differ"
    return got[0]


def goertzel_call(c, x, rate, freqs, form="dev", runs=2):
    batch, n = x.shape
    f = np.ascontiguousarray(freqs, np.float32)
    arena = Arena("host" if form == "host" else "cuda", f"goertzel {form} n={n} batch={batch} nfreq={f.size}")
    off = 4 if form == "dev_off" else 0
    xin = arena.input(x, align_off=off, row_bytes=4 * n)
    out = arena.output(4 * f.size * batch, align_off=off, row_bytes=4 * f.size)
    fn = c.lib.kofft_hip_goertzel_f32 if form == "host" else c.lib.kofft_hip_dev_goertzel_f32
    got = []
    for _ in range(runs):
        _ok(c, fn(c.h, C.c_void_p(xin.addr), C.c_void_p(out.addr), n, batch, C.c_float(rate), C.c_void_p(f.ctypes.data), f.size))
        _ok(c, c.lib.kofft_hip_synchronize(c.h))
        arena.verify()
        got.append(arena.read(out, np.float32, (batch, f.size)))
        arena.restore(out)
    for g in got[1:]:
        assert bits_equal(got[0], g), f"{arena.what}: two runs of the same call differ"
    return got[0]


def _all_routes(c, x, m, w, a, what, form="dev"):
    """Every route, each twice (the second run of route 2 and of the default finds the table cached): one result, the oracle's."""
    want = so.czt(x, m, w, a)
    try:
        for mode in (1, 2, 0):
            c.route(mode)
            assert_rows_equal(czt_call(c, x, m, w, a, form), want, f"{what} route {mode}", nan_safe=True)
    finally:
        c.route(0)


# ---- chirp-Z ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n,m,batch,name", _czt_cases())
def test_czt_every_route_is_the_oracle(ctx, n, m, batch, name):
    w, a = so.param_sets(m)[name]
    x = seeded(15000 + 31 * n + 7 * m + batch).uniform(-1, 1, (batch, n)).astype(np.float32)
    _all_routes(ctx, x, m, w, a, f"{name} n={n} m={m} batch={batch}")


@gpu
def test_czt_full_size(ctx):
    n = m = 4096
    w, a = so.param_sets(m)["dft"]
    x = seeded(15900).uniform(-1, 1, (8, n)).astype(np.float32)
    _all_routes(ctx, x, m, w, a, "dft n=m=4096 batch=8")
    assert ctx.lib.kofft_hip_release_scratch(ctx.h) == 0  # the 128 MiB table goes back


@gpu
@pytest.mark.parametrize("name,n,m,batch", [("dft", 100, 100, 70), ("zoom", 257, 129, 65), ("spiral", 1024, 129, 70), ("a_zero", 65, 33, 64),
                                            ("grow", 257, 65, 66), ("spiral", 1024, 31, 3), ("grow", 257, 300, 2)])
def test_czt_parameter_sets(ctx, name, n, m, batch):
    """(c) the decaying spiral runs wnk through subnormals into zero -- a flushed subnormal changes bits here; (d) a = 0 takes the
    denom == 0 branch; (e) |w| = 1.5 overflows to Inf and then NaN."""
    w, a = so.param_sets(m)[name]
    x = seeded(16000 + n + m).uniform(-1, 1, (batch, n)).astype(np.float32)
    want = so.czt(x, m, w, a)
    if name == "spiral":
        t = so.czt_table(n, m, w, a)
        assert np.any((t != 0) & (np.abs(t) < np.finfo(np.float32).tiny)) and np.any(t[-1] == 0), "the case no longer reaches subnormals"
    if name == "grow":
        assert np.isnan(want).any() and np.isinf(so.czt_table(n, m, w, a)).any()
    _all_routes(ctx, x, m, w, a, f"{name} n={n} m={m} batch={batch}")


@gpu
def test_czt_special_inputs(ctx):
    n, m, batch = 100, 65, 66
    x = seeded(16500).uniform(-1, 1, (batch, n)).astype(np.float32)
    x[3, 7], x[3, 50], x[64, 0], x[65, 99] = np.nan, np.inf, -np.inf, 3e38
    x[10] = 1e-41
    x[11] = -0.0
    w, a = so.param_sets(m)["zoom"]
    _all_routes(ctx, x, m, w, a, "special inputs")


@gpu
def test_czt_table_cache_evicts_and_rebuilds(hiplib):
    """Five (w, a) on one context through the table route: the fifth evicts the first, which then reproduces its bytes."""
    c = Ctx(hiplib)
    try:
        c.route(2)
        n, m, batch = 65, 33, 70
        x = seeded(16600).uniform(-1, 1, (batch, n)).astype(np.float32)
        sets = [so.param_sets(m)[k] for k in ("dft", "zoom", "spiral", "a_zero", "grow")]
        first = [czt_call(c, x, m, w, a) for w, a in sets]
        for (w, a), got in zip(sets, first):
            assert_rows_equal(got, so.czt(x, m, w, a), "cache fill", nan_safe=True)
        again = czt_call(c, x, m, *sets[0])
        assert bits_equal(again, first[0])
        for (w, a), got in zip(reversed(sets), reversed(first)):  # and every one of them once more, in another order
            assert bits_equal(czt_call(c, x, m, w, a, runs=1), got)
    finally:
        c.close()


@gpu
@pytest.mark.parametrize("form", ["host", "dev_off"])
def test_czt_pointer_forms(ctx, form):
    for n, m, batch in [(17, 5, 3), (100, 64, 65), (65, 129, 129), (0, 4, 3)]:
        w, a = so.param_sets(m)["zoom"]
        x = seeded(16700 + n).uniform(-1, 1, (batch, n)).astype(np.float32)
        _all_routes(ctx, x, m, w, a, f"{form} n={n} m={m} batch={batch}", form)


@gpu
def test_czt_overlap_and_python(ctx, fft32):
    import torch

    import kofft_amd
    from kofft_amd import czt

    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    assert ctx.lib.kofft_hip_dev_czt_f32(ctx.h, C.c_void_p(p), C.c_void_p(p + 4 * 8), 16, 4, 1.0, 0.0, 1.0, 0.0, 2) == 6
    assert ctx.lib.kofft_hip_set_czt_route(ctx.h, 3) == 6 and ctx.lib.kofft_hip_set_czt_route(ctx.h, -1) == 6
    x = seeded(16800).uniform(-1, 1, (5, 40)).astype(np.float32)
    w, a = so.param_sets(9)["zoom"]
    want = so.czt(x, 9, w, a)
    assert bits_equal(czt.czt_f32(x, 9, w, a, fft=fft32), want)
    assert bits_equal(czt.czt_f32(x[0], 9, w, a, fft=fft32), want[0])
    t = fft32.czt(torch.from_numpy(x).cuda(), 9, w, a)
    fft32.synchronize()
    assert bits_equal(t.cpu().numpy(), want)
    y = czt.czt_f32(np.array([0, 1], np.float32), 2, (0.0, 1.0), (0.5, 0.0), fft=fft32)  # czt.rs:74-81
    assert abs(y[0] - 2) < 1e-5 and abs(y[1] - 2j) < 1e-5
    assert not czt.czt_f32(np.zeros(0, np.float32), 3, w, a, fft=fft32).view(np.float32).any()
    with pytest.raises(kofft_amd.DeviceError):
        fft32.czt(x, 5000, w, a)


# ---- Goertzel -----------------------------------------------------------------------------------------------------------------------------
GZ_CHUNK = 32
GZ_NS = [1, 2, 3, GZ_CHUNK - 1, GZ_CHUNK, GZ_CHUNK + 1, 100, 1000, 4099]
RATE = 8000.0
BASE_FREQS = [1000.0, 0.0, 4000.0, 9000.0, -500.0, 697.0, 1633.0, 3999.5]  # the reference's tone, DC, Nyquist, above the rate, negative


def _freqs(nfreq):
    if nfreq <= len(BASE_FREQS):
        return np.array(BASE_FREQS[:nfreq], np.float32)
    return np.concatenate([np.array(BASE_FREQS, np.float32), np.linspace(-1000.0, 12000.0, nfreq - len(BASE_FREQS)).astype(np.float32)])


def _gz_cases():
    """Every n against every nfreq, the batch cycling through 1, 3 and one workgroup's rows - 1 / +0 / +1 (256 // nfreq); batch 1000 at
    the lengths where the oracle stays quick."""
    cases = []
    for nfreq in (1, 3, 8, 65):
        rows = 256 // nfreq
        batches = [1, 3, rows - 1, rows, rows + 1]
        for j, n in enumerate(GZ_NS):
            cases.append((n, batches[(j + nfreq) % 5], nfreq))
        cases.append((100, 1000, nfreq))
        cases.append((GZ_CHUNK + 1, batches[3], nfreq))
    # beyond the issue's list, the two paths it does not reach: more than 256 frequencies (several frequency chunks per row group, one
    # row per workgroup) and more row groups than the grid's 65535 (the group-stride loop), each at the smallest shape that takes it
    cases += [(33, 3, 300), (4, 2, 1024), (2, 65600, 256)]
    return cases


@gpu
@pytest.mark.parametrize("n,batch,nfreq", _gz_cases())
def test_goertzel_is_the_oracle(ctx, n, batch, nfreq):
    x = seeded(17000 + 13 * n + batch + nfreq).uniform(-1, 1, (batch, n)).astype(np.float32)
    f = _freqs(nfreq)
    want = so.goertzel(x, RATE, f)
    for form in ("dev", "dev_off", "host") if batch < 65536 else ("dev",):
        assert_rows_equal(goertzel_call(ctx, x, RATE, f, form), want, f"{form} n={n} batch={batch} nfreq={nfreq}", nan_safe=True)


@gpu
def test_czt_sum_route_beyond_the_grid_limit(ctx):
    """czt_recur_kernel<SUM> with more row groups than the grid's 65535 (m >= 256: one row per workgroup): the group-stride loop."""
    n, m, batch = 2, 256, 65600
    w, a = so.param_sets(m)["zoom"]
    x = seeded(16900).uniform(-1, 1, (batch, n)).astype(np.float32)
    try:
        ctx.route(1)
        assert_rows_equal(czt_call(ctx, x, m, w, a, runs=1), so.czt(x, m, w, a), "sum route, 65600 row groups", nan_safe=True)
    finally:
        ctx.route(0)


@gpu
def test_goertzel_special_rows_leave_their_neighbours_alone(ctx):
    x = seeded(17500).uniform(-1, 1, (40, 100)).astype(np.float32)
    x[17, 3], x[17, 60], x[17, 99] = np.nan, np.inf, -np.inf
    x[5] = 1e-41
    f = _freqs(8)
    want = so.goertzel(x, RATE, f)
    assert np.isnan(want[17]).all() and not np.isnan(want[[16, 18]]).any()
    for form in ("dev", "host"):
        assert_rows_equal(goertzel_call(ctx, x, RATE, f, form), want, form, nan_safe=True)


@gpu
def test_goertzel_power_that_rounds_negative(ctx):
    """Seed 14011 at n = 100, 64 rows: the oracle's power of one (row, frequency) rounds below zero, so the reference returns NaN from
    finite samples (found among the seeds, not constructed)."""
    x = seeded(14011).uniform(-1, 1, (64, 100)).astype(np.float32)
    f = np.array([0.0, 4000.0, 1000.0], np.float32)
    want = so.goertzel(x, RATE, f)
    assert np.isnan(want).sum() == 1
    assert_rows_equal(goertzel_call(ctx, x, RATE, f), want, "negative power", nan_safe=True)


@gpu
def test_goertzel_reference_tone_nan_rate_and_python(ctx, fft32):
    import torch

    import kofft_amd
    from kofft_amd import goertzel

    i = np.arange(100, dtype=np.float32)
    sig = np.sin(np.float32(2.0) * np.float32(np.pi) * np.float32(1000.0) * i / np.float32(8000.0)).astype(np.float32)
    mag = goertzel.goertzel_f32(sig, 8000.0, 1000.0, fft=fft32)  # goertzel.rs:65-76
    assert isinstance(mag, float) and mag > 0.0 and np.float32(mag).tobytes() == np.float32(so.goertzel_scalar(sig, 8000.0, 1000.0)).tobytes()
    x = seeded(17600).uniform(-1, 1, (7, 33)).astype(np.float32)
    f = _freqs(3)
    want = so.goertzel(x, RATE, f)
    assert bits_equal(goertzel.goertzel_f32(x, RATE, f, fft=fft32), want)
    t = fft32.goertzel(torch.from_numpy(x).cuda(), RATE, f)
    fft32.synchronize()
    assert bits_equal(t.cpu().numpy(), want)
    assert np.isnan(goertzel_call(ctx, x, float("nan"), f)).all()  # a NaN rate passes `<= 0.0`: NaN coefficients, NaN results
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    fp = C.c_void_p(f.ctypes.data)
    assert ctx.lib.kofft_hip_dev_goertzel_f32(ctx.h, C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr() + 64), 33, 7, C.c_float(RATE), fp, 3) == 6
    with pytest.raises(kofft_amd.FftError):
        fft32.goertzel(x, 0.0, f)


@gpu
def test_goertzel_frequency_sets_change_between_device_calls(hiplib):
    """The device-pointer form keeps one coefficient buffer per context: six sets one after the other, each then once more (no upload),
    and a set of another length, all without a synchronisation of the caller's in between changing a result."""
    c = Ctx(hiplib)
    try:
        x = seeded(17700).uniform(-1, 1, (9, 70)).astype(np.float32)
        sets = [np.array([100.0 * j, 50.0 * j + 3], np.float32) for j in range(1, 7)]
        first = [goertzel_call(c, x, RATE, f, runs=1) for f in sets]
        for f, got in zip(sets, first):
            assert_rows_equal(got, so.goertzel(x, RATE, f), "cache fill", nan_safe=True)
            assert bits_equal(goertzel_call(c, x, RATE, f, runs=1), got)
        wide = _freqs(300)
        assert_rows_equal(goertzel_call(c, x, RATE, wide, runs=1), so.goertzel(x, RATE, wide), "300 after 2", nan_safe=True)
        assert_rows_equal(goertzel_call(c, x, RATE, sets[0], runs=1), first[0], "2 after 300", nan_safe=True)
        assert c.lib.kofft_hip_release_scratch(c.h) == 0
        assert_rows_equal(goertzel_call(c, x, RATE, sets[0], runs=1), first[0], "after release_scratch", nan_safe=True)
    finally:
        c.close()


# ---- a non-default stream -------------------------------------------------------------------------------------------------------------------
@gpu
def test_both_families_on_a_non_default_stream(hiplib):
    import torch

    c = Ctx(hiplib)
    try:
        s = torch.cuda.Stream()
        assert hiplib.kofft_hip_set_stream(c.h, C.c_void_p(s.cuda_stream)) == 0
        x = seeded(17800).uniform(-1, 1, (130, 100)).astype(np.float32)
        w, a = so.param_sets(65)["zoom"]
        _all_routes(c, x, 65, w, a, "stream")
        assert_rows_equal(goertzel_call(c, x, RATE, _freqs(8)), so.goertzel(x, RATE, _freqs(8)), "stream", nan_safe=True)
        assert hiplib.kofft_hip_set_stream(c.h, None) == 0
        assert_rows_equal(czt_call(c, x, 65, w, a), so.czt(x, 65, w, a), "back on the own stream (cached table)", nan_safe=True)
    finally:
        c.close()


# ---- guard bands: the case table ---------------------------------------------------------------------------------------------------------------
def _band_czt(form):
    def run(c):
        for n, m, batch in [(100, 65, 129), (16, 3, 5)]:
            x = seeded(18000 + n).uniform(-1, 1, (batch, n)).astype(np.float32)
            w, a = so.param_sets(m)["zoom"]
            _all_routes(c, x, m, w, a, f"bands {form}", form)
    return run


def _band_goertzel(form):
    def run(c):
        for n, batch, nfreq in [(33, 257, 1), (100, 33, 8), (4099, 4, 65)]:
            x = seeded(18100 + n).uniform(-1, 1, (batch, n)).astype(np.float32)
            assert_rows_equal(goertzel_call(c, x, RATE, _freqs(nfreq), form), so.goertzel(x, RATE, _freqs(nfreq)), f"bands {form}", nan_safe=True)
    return run


BAND_CASES = {
    "kofft_hip_czt_f32": _band_czt("host"),
    "kofft_hip_dev_czt_f32": _band_czt("dev_off"),
    "kofft_hip_goertzel_f32": _band_goertzel("host"),
    "kofft_hip_dev_goertzel_f32": _band_goertzel("dev_off"),
}


@gpu
@pytest.mark.parametrize("name", sorted(BAND_CASES))
def test_guard_bands(ctx, name):
    """Two runs inside bands (czt_call / goertzel_call): bands intact, const inputs intact, outputs bit-exact and equal."""
    BAND_CASES[name](ctx)


def test_every_new_entry_point_with_data_pointers_has_a_guard_band_case():
    """Every function of the chirp-Z / Goertzel section of include/kofft_hip.h that takes a context and data pointers is in BAND_CASES
    (the host-only table functions write caller memory on the CPU: tests/test_spectral_cpu.py and the sanitizer program cover them)."""
    text = (ROOT / "include" / "kofft_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"int\s+(kofft_hip_\w*(?:czt|goertzel)\w*)\s*\(([^;]*)\);", text)
    assert len(protos) == 7, [p[0] for p in protos]
    need = {name for name, args in protos if "kofft_hip_ctx" in args and re.search(r"float\s*\*", args)}
    assert need == set(BAND_CASES), sorted(need ^ set(BAND_CASES))
