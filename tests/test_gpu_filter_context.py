"""The filter and lapped families (resample, sosfilt, sosfilt_scan, convolve_bank, the fast DCT-IV, mdct, imdct) on SHARED context
state: the composed routes' scratch (ctx->real_tmp for the bank's spectra and frames, the scan's chunk states and the
composed DCT-IV's complex rows; ctx->rows_tmp for the IMDCT's frames, with a nested composed DCT-IV on real_tmp), the table cache
(twiddles, Bluestein, the DCT-IV's own kind), stream switches, release_scratch, hipGraph capture and two threads at once.  The
tests mirror tests 1-6 of tests/test_gpu_rowwise_context.py; every output is compared bit for bit with the family's oracle, and the
host calls run twice."""
import threading

import numpy as np
import pytest

import mdct_oracle as mo
from conftest import bits_equal, seeded
from convolve_bank_oracle import convolve_bank_ref
from convolve_oracle import convolve_ref
from resample_oracle import resample_ref
from rowcheck import assert_rows_equal
from sosfilt_oracle import cascade, sosfilt_ref
from sosfilt_scan_oracle import TILE as T
from sosfilt_scan_oracle import sosfilt_scan_ref

pytestmark = pytest.mark.gpu

F = np.float32
PAD = 4
KNOB = "KOFFT_HIP_SCRATCH_CHUNK_MB"


def _x(shape, seed):
    return seeded(seed).uniform(-1, 1, shape).astype(F)


def _window(n, seed):
    return seeded(seed).uniform(0.1, 1.0, 2 * n).astype(F)


def _twice(fn, *args, **kw):
    a = fn(*args, **kw)
    b = fn(*args, **kw)
    pa, pb = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    for u, v in zip(pa, pb):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes(), f"{fn.__name__}: two runs differ"
    return a


# ---- device-form operations: inputs uploaded up front, outputs read after one synchronisation -----------------------------------
class Op:
    """One _dev call on fresh device buffers: enqueue(f) on the context's current stream, check() against the oracle afterwards.
    `want()` is one array or a list of arrays that lie one behind the other in the output buffer."""

    def __init__(self, what, inputs, out_floats, call, want, out_view=None):
        import torch

        self.what = what
        self.ins = [torch.from_numpy(np.ascontiguousarray(a, F).reshape(-1)).cuda() for a in inputs]
        self.out = torch.full((out_floats + PAD,), 7.0, dtype=torch.float32, device="cuda")  # PAD floats behind the output: checked by result()
        self.out_floats, self.fill = out_floats, 7.0
        self.call, self.want, self.out_view = call, want, out_view

    def enqueue(self, f):
        self.call(f, *[t.data_ptr() for t in self.ins], self.out.data_ptr())

    def result(self):
        assert bool((self.out[self.out_floats:] == self.fill).all()), f"{self.what}: the padding behind the output was written"
        got = self.out[:self.out_floats].cpu().numpy()
        return self.out_view(got) if self.out_view else got

    def check(self):
        want = self.want()
        got = self.result()
        if isinstance(want, list):
            o = 0
            for l, w in enumerate(want):
                assert_rows_equal(got[o:o + w.size].reshape(w.shape[0], -1), w.reshape(w.shape[0], -1), f"{self.what} part {l}")
                o += w.size
        else:
            assert_rows_equal(got.reshape(want.shape[0], -1), want.reshape(want.shape[0], -1), self.what)


def op_resample(rows, nx, nh, up, down, seed):
    x, h = _x((rows, nx), seed), _x((nh,), seed + 1)
    out_len = -(-((nx - 1) * up + nh) // down)
    return Op(f"resample {up}/{down} rows={rows} nx={nx} nh={nh}", [x, h], rows * out_len,
              lambda f, dx, dh, o: f.resample_dev(dx, rows, nx, dh, nh, up, down, 0, o, out_len), lambda: resample_ref(x, h, up, down, 0, out_len))


def op_sosfilt(rows, nx, sections, seed, reverse=False):
    x, zi, sos = _x((rows, nx), seed), _x((rows, sections, 2), seed + 1), cascade(sections, seed)
    na = rows * nx

    def call(f, dx, dsos, dzi, o):
        f.sosfilt_dev(dx, rows, nx, dsos, sections, dzi, o + 4 * na, o, reverse=reverse)

    return Op(f"sosfilt rows={rows} nx={nx} sections={sections}", [x, sos, zi], na + rows * sections * 2, call,
              lambda: list(sosfilt_ref(sos, x, zi, reverse)))


def op_scan(rows, nx, sections, chunk, seed, reverse=False):
    x, zi, sos = _x((rows, nx), seed), _x((rows, sections, 2), seed + 1), cascade(sections, seed)
    na = rows * nx

    def call(f, dx, dsos, dzi, o):
        f.sosfilt_scan_dev(dx, rows, nx, dsos, sections, dzi, o + 4 * na, chunk, o, reverse=reverse)

    return Op(f"sosfilt_scan rows={rows} nx={nx} sections={sections} chunk={chunk}", [x, sos, zi], na + rows * sections * 2, call,
              lambda: list(sosfilt_scan_ref(sos, x, chunk, zi, reverse)))


def op_bank(block, rows, nx, nh, filters, kind, seed, correlate=False):
    x, h = _x((rows, nx), seed), _x((filters, nh), seed + 1)
    full = nx + nh - 1
    cplx = kind == "complex"

    def call(f, dx, dh, o):
        f.convolve_bank_dev(dx, rows, nx, dh, filters, nh, o, block=block, correlate=correlate, out=kind)

    return Op(f"convolve_bank block={block} rows={rows} nx={nx} nh={nh} filters={filters} {kind}", [x, h], rows * filters * full * (2 if cplx else 1),
              call, lambda: convolve_bank_ref(x, h, block, correlate, kind).reshape(rows * filters, full),
              (lambda g: g.view(np.complex64).reshape(rows * filters, full)) if cplx else None)


def op_dct4(n, b, seed):
    u = _x((b, n), seed)
    return Op(f"dct4_fast n={n} b={b}", [u], b * n, lambda f, i, o: f.dct4_fast_dev(i, o, n, b), lambda: mo.dct4_ref(u))


def op_mdct(n, rows, nx, seed, lead=None):
    x, w = _x((rows, nx), seed), _window(n, seed + 1)
    lead = n if lead is None else lead
    frames = -(-(nx + lead) // n)
    return Op(f"mdct n={n} rows={rows} nx={nx} lead={lead}", [x, w], rows * frames * n,
              lambda f, dx, dw, o: f.mdct_dev(dx, rows, nx, nx, dw, n, lead, o, frames),
              lambda: mo.mdct_ref(x, w, lead, frames).reshape(rows * frames, n))


def op_imdct(n, rows, frames, seed, scale=0.37):
    X, w = _x((rows, frames, n), seed), _window(n, seed + 1)
    full = (frames + 1) * n
    return Op(f"imdct n={n} rows={rows} frames={frames}", [X, w], rows * full,
              lambda f, dx, dw, o: f.imdct_dev(dx, rows, frames, dw, n, scale, o, 0, full), lambda: mo.imdct_ref(X, w, scale))


def _streams():
    import torch

    return torch.cuda.Stream(), torch.cuda.Stream()


# ---- 1. stream switching over the shared scratch ----------------------------------------------------------------------------------
def test_stream_switching_over_real_tmp_and_rows_tmp(oracle):
    """The composed bank (its spectra and frames side by side in real_tmp), the scan (its chunk states there), the composed DCT-IV (its
    complex rows there), the MDCT and the IMDCT (its frames in rows_tmp, a nested composed DCT-IV on real_tmp) on one context,
    alternating two streams with no host synchronisation.  The sizes are ordered so that real_tmp must grow at the block-8192 bank
    (0.9 MiB after 57 KiB) and again at dct4 N = 16384 (2.6 MiB) and rows_tmp at the second imdct (1.3 MiB after 58 KiB), while work on
    the other stream may still read the old buffer; then they shrink again.  Two passes: every op equals the oracle and its own first
    pass."""
    import torch

    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    f.set_convolve_bank_fused(False)
    f.set_mdct_fused(False)
    s1, s2 = _streams()
    ops = [op_bank(64, 3, 500, 9, 2, "real", 100), op_scan(4, 3000, 3, T, 102), op_dct4(240, 5, 104), op_mdct(960, 2, 5000, 105),
           op_imdct(960, 2, 7, 107), op_bank(8192, 2, 20000, 100, 2, "magnitude", 109), op_scan(40, 4000, 9, T, 111, reverse=True),
           op_dct4(16384, 40, 113), op_mdct(960, 30, 9000, 114), op_imdct(960, 30, 11, 116), op_bank(64, 5, 300, 64, 3, "complex", 118),
           op_dct4(240, 33, 120), op_scan(3, 2049, 17, T, 121)]
    torch.cuda.synchronize()
    for rep in range(2):
        for k, op in enumerate(ops):
            f.set_stream((s1 if k % 2 == 0 else s2).cuda_stream)
            op.enqueue(f)
        torch.cuda.synchronize()
        first = [op.result().tobytes() for op in ops] if rep == 0 else first
    for op, b in zip(ops, first):
        op.check()
        assert op.result().tobytes() == b, f"{op.what}: the second pass differs from the first"
    f.set_stream(0)
    f.close()


# ---- 2. tables built on one stream, used on another --------------------------------------------------------------------------------
def test_tables_built_on_one_stream_used_on_another(oracle):
    """The first dct4_fast of a size (the DCT-IV table and the twiddles, or the Bluestein tables, built and uploaded) and the first
    convolve_bank of a block on s1, the next call of that size on s2 without a sync: N = 2048 fused, N = 960 composed (a Bluestein
    transform of 480 points), block 512 fused and block 16 (below the fused range)."""
    import torch

    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    s1, s2 = _streams()
    pairs = [(op_dct4(2048, 9, 200), op_dct4(2048, 9, 201)), (op_dct4(960, 7, 202), op_dct4(960, 7, 203)),
             (op_bank(512, 3, 3000, 100, 2, "real", 204), op_bank(512, 3, 3000, 100, 2, "real", 206)),
             (op_bank(16, 3, 100, 5, 2, "complex", 208), op_bank(16, 3, 100, 5, 2, "complex", 210))]
    torch.cuda.synchronize()
    for a, b in pairs:
        f.set_stream(s1.cuda_stream)
        a.enqueue(f)
        f.set_stream(s2.cuda_stream)
        b.enqueue(f)
    torch.cuda.synchronize()
    for a, b in pairs:
        a.check()
        b.check()
    f.set_stream(0)
    f.close()


# ---- 3. release_scratch between families ------------------------------------------------------------------------------------------
def test_release_scratch_between_families(oracle):
    """release_scratch between the composed bank, the scan, the IMDCT and a fused MDCT (which uses no scratch): unchanged output, twice."""
    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    f.set_convolve_bank_fused(False)
    x1, h1 = _x((5, 3000), 300), _x((3, 65), 301)
    x2, zi2, sos2 = _x((6, 4000), 302), _x((6, 9, 2), 303), cascade(9, 3)
    X3, w3 = _x((4, 9, 1024), 304), _window(1024, 305)
    x4, w4 = _x((3, 5000), 306), _window(512, 307)
    w1 = convolve_bank_ref(x1, h1, 256, True, "magnitude")
    w2 = sosfilt_scan_ref(sos2, x2, 2 * T, zi2)
    w3r = mo.imdct_ref(X3, w3, 2.0 / 1024)
    w4r = mo.mdct_ref(x4, w4, 512, -(-5000 // 512) + 1)
    for rep in range(2):
        got = _twice(f.convolve_bank_rows, x1, h1, block=256, correlate=True, out="magnitude")
        assert_rows_equal(got.reshape(15, -1), w1.reshape(15, -1), "composed convolve_bank")
        f.release_scratch()
        y, zf = _twice(f.sosfilt_scan_rows, x2, sos2, 2 * T, zi=zi2, zf=True)
        assert_rows_equal(y, w2[0], "sosfilt_scan")
        assert_rows_equal(zf.reshape(6, -1), w2[1].reshape(6, -1), "sosfilt_scan final states")
        f.release_scratch()
        assert_rows_equal(_twice(f.imdct_rows, X3, w3), w3r, "imdct")
        f.release_scratch()
        got = _twice(f.mdct_rows, x4, w4)
        assert_rows_equal(got.reshape(-1, 512), w4r.reshape(-1, 512), "fused mdct")
        f.release_scratch()
    f.close()


# ---- 4. every family interleaved with the older users of the same scratch -------------------------------------------------------------
def test_families_interleaved_with_older_users_of_the_scratch(oracle):
    """One context under a 1 MiB scratch chunk: the five families between a composed rfft (n = 3000) and an STFT with a 1000-point
    window, sizes growing and shrinking over three rounds and the bank's and the DCT-IV's routes alternating; at the end the
    overlap-save convolve, which shares k_convolve_f32.hip and the scratch layout with the bank."""
    import kofft_amd

    mp = pytest.MonkeyPatch()
    mp.setenv(KNOB, "1")
    try:
        f = kofft_amd.HipFftImpl(np.float32)
    finally:
        mp.undo()
    rng = seeded(400)
    sig = rng.uniform(-1, 1, 30000).astype(F)
    win = rng.uniform(0.1, 1, 1000).astype(F)
    frames = -(-sig.size // 250)
    h = _x((31,), 401)
    bank = _x((3, 65), 402)
    for rep, (b_small, b_big) in enumerate([(3, 200), (150, 7), (2, 40)]):
        f.set_convolve_bank_fused(rep % 2 == 1)
        f.set_mdct_fused(rep % 2 == 1)
        xr = _x((b_big, 3000), 410 + rep)
        assert bits_equal(f.rfft_batch(xr), oracle.rfft(xr, None)), "composed rfft n=3000"
        x = _x((b_small, 1000), 420 + rep)
        assert_rows_equal(_twice(f.resample_rows, x, h, 3, 2), resample_ref(x, h, 3, 2, 0, -(-(999 * 3 + 31) // 2)), "resample 3/2")
        xs, zs, sos = _x((b_big, 300), 430 + rep), _x((b_big, 3, 2), 435 + rep), cascade(3, rep)
        y, zf = _twice(f.sosfilt_rows, xs, sos, zi=zs, zf=True)
        wy, wz = sosfilt_ref(sos, xs, zs)
        assert_rows_equal(y, wy, "sosfilt")
        assert_rows_equal(zf.reshape(b_big, -1), wz.reshape(b_big, -1), "sosfilt final states")
        xc, zc, sos9 = _x((b_small, 3000), 440 + rep), _x((b_small, 9, 2), 445 + rep), cascade(9, rep)
        y, zf = _twice(f.sosfilt_scan_rows, xc, sos9, T, zi=zc, zf=True, reverse=bool(rep % 2))
        wy, wz = sosfilt_scan_ref(sos9, xc, T, zc, bool(rep % 2))
        assert_rows_equal(y, wy, "sosfilt_scan")
        assert_rows_equal(zf.reshape(b_small, -1), wz.reshape(b_small, -1), "sosfilt_scan final states")
        xb = _x((b_small, 2000), 450 + rep)
        got = _twice(f.convolve_bank_rows, xb, bank, block=256, out="magnitude")
        assert_rows_equal(got.reshape(b_small * 3, -1), convolve_bank_ref(xb, bank, 256, False, "magnitude").reshape(b_small * 3, -1), "convolve_bank")
        assert bits_equal(f.stft_into(sig, win, 250, frames), oracle.stft(sig, win, 250, frames)), "stft win=1000"
        u = _x((b_big, 240), 460 + rep)
        assert_rows_equal(_twice(f.dct4_fast_batch, u), mo.dct4_ref(u), "dct4_fast n=240")
        xm, wm = _x((b_small, 5000), 470 + rep), _window(960, 475 + rep)
        got = _twice(f.mdct_rows, xm, wm)
        assert_rows_equal(got.reshape(-1, 960), mo.mdct_ref(xm, wm, 960, -(-5000 // 960) + 1).reshape(-1, 960), "mdct N=960")
        Xi, wi = _x((b_small, 6, 1024), 480 + rep), _window(1024, 485 + rep)
        assert_rows_equal(_twice(f.imdct_rows, Xi, wi), mo.imdct_ref(Xi, wi, 2.0 / 1024), "imdct N=1024")
    f.set_convolve_fused(False)
    xv, hv = _x((17, 20000), 490), _x((100,), 491)
    assert_rows_equal(_twice(f.convolve_rows, xv, hv, block=1024), convolve_ref(xv, hv, 1024), "overlap-save convolve, composed, in chunks")
    f.close()


# ---- 5. hipGraph capture -------------------------------------------------------------------------------------------------------
def test_filter_device_calls_can_be_captured_into_a_hip_graph(oracle):
    """After a warm-up (tables uploaded, scratch grown) every family's _dev call is kernel launches on the context's stream and nothing
    else: ensure() returns at once when the buffer is large enough and a cached table is one find (host_cache.h).  Captured in
    sequence on one side stream (a linear graph) -- plain and tiled resample and sosfilt, the scan, the fused and the composed bank,
    dct4_fast, mdct and imdct -- nothing runs before replay, and two replays give the direct calls' bytes, which are the oracle's."""
    import torch

    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    s = torch.cuda.Stream()
    f.set_stream(s.cuda_stream)
    # (route, op): route set on the context right before the call -- a host-side switch, read at enqueue time
    plan = [
        ("resample_plain", op_resample(3, 700, 31, 3, 2, 500)), ("resample_tiled", op_resample(3, 700, 31, 3, 2, 502)),
        ("sosfilt_plain", op_sosfilt(70, 2 * T + 5, 9, 504)), ("sosfilt_tiled", op_sosfilt(70, 2 * T + 5, 9, 506)),
        ("scan", op_scan(3, 3000, 9, T, 508)),
        ("bank_fused", op_bank(256, 3, 2000, 65, 2, "magnitude", 510)), ("bank_composed", op_bank(256, 3, 2000, 65, 2, "magnitude", 512)),
        ("dct_fused", op_dct4(1024, 9, 514)), ("dct_composed", op_dct4(1024, 9, 515)), ("dct_composed", op_dct4(240, 9, 516)),
        ("dct_fused", op_mdct(512, 3, 4000, 517)), ("dct_composed", op_mdct(512, 3, 4000, 519)),
        ("dct_fused", op_imdct(512, 3, 7, 521)), ("dct_composed", op_imdct(512, 3, 7, 523)), ("dct_composed", op_imdct(240, 2, 5, 525)),
    ]

    def route(r):
        f.set_resample_tiled(0 if r == "resample_plain" else 2)
        f.set_sosfilt_tiled(0 if r == "sosfilt_plain" else 2)
        f.set_convolve_bank_fused(r != "bank_composed")
        f.set_mdct_fused(r != "dct_composed")

    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for r, op in plan:  # warm-up, outside the capture
            route(r)
            op.enqueue(f)
    torch.cuda.synchronize()
    direct_bytes = [op.result().tobytes() for _, op in plan]
    for _, op in plan:
        op.out.fill_(0.0)
        op.fill = 0.0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for r, op in plan:
            route(r)
            op.enqueue(f)
    torch.cuda.synchronize()
    for _, op in plan:
        assert float(op.out.abs().sum()) == 0.0, f"{op.what}: ran during the capture"
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    for (r, op), b in zip(plan, direct_bytes):
        assert op.result().tobytes() == b, f"{op.what} ({r}): the replay differs from the direct call"
        op.check()
    f.set_stream(0)
    f.close()


# ---- 6. two threads, fresh contexts, first uses at the same time --------------------------------------------------------------
def test_two_threads_first_uses_at_the_same_time(oracle):
    """One thread makes first-use dct4_fast, mdct and imdct calls (the DCT-IV, twiddle and Bluestein tables are built) while the other
    makes first-use resample, sosfilt and convolve_bank calls, each on a fresh context.  Every result must be the oracle's.  A worker
    that fails before the barrier breaks it, so the other one cannot wait forever."""
    import kofft_amd

    errors = []
    barrier = threading.Barrier(2, timeout=120)

    def lapped_worker():
        try:
            f = kofft_amd.HipFftImpl(np.float32)
            barrier.wait()
            for n, b in ((4096, 5), (960, 9), (128, 300)):
                u = _x((b, n), 600 + n)
                assert_rows_equal(_twice(f.dct4_fast_batch, u), mo.dct4_ref(u), f"dct4_fast n={n}")
                x, w = _x((3, 5 * n + 3), 610 + n), _window(n, 620 + n)
                X = _twice(f.mdct_rows, x, w)
                want = mo.mdct_ref(x, w, n, X.shape[1])
                assert_rows_equal(X.reshape(-1, n), want.reshape(-1, n), f"mdct N={n}")
                assert_rows_equal(_twice(f.imdct_rows, want, w), mo.imdct_ref(want, w, 2.0 / n), f"imdct N={n}")
            f.close()
        except Exception as e:  # noqa: BLE001 -- reported below, in the main thread
            barrier.abort()
            errors.append(repr(e))

    def filter_worker():
        try:
            f = kofft_amd.HipFftImpl(np.float32)
            barrier.wait()
            for k, (block, nh) in enumerate(((2048, 300), (128, 33), (8192, 1000))):
                x, h = _x((3, 9000), 630 + k), _x((2, nh), 640 + k)
                got = _twice(f.convolve_bank_rows, x, h, block=block, out="complex")
                assert_rows_equal(got.reshape(6, -1), convolve_bank_ref(x, h, block, False, "complex").reshape(6, -1), f"convolve_bank block={block}")
                xr, hr = _x((5, 2000), 650 + k), _x((4 * (k + 2) + 1,), 660 + k)
                assert_rows_equal(_twice(f.resample_rows, xr, hr, k + 2, 3), resample_ref(xr, hr, k + 2, 3, 0, -(-(1999 * (k + 2) + hr.size) // 3)),
                                  f"resample {k + 2}/3")
                xs, sos = _x((70, 500), 670 + k), cascade(9, k)
                assert_rows_equal(_twice(f.sosfilt_rows, xs, sos), sosfilt_ref(sos, xs)[0], "sosfilt")
            f.close()
        except Exception as e:  # noqa: BLE001
            barrier.abort()
            errors.append(repr(e))

    a, b = threading.Thread(target=lapped_worker, daemon=True), threading.Thread(target=filter_worker, daemon=True)
    a.start(); b.start(); a.join(300); b.join(300)
    assert not (a.is_alive() or b.is_alive()), "a worker did not finish within 300 s"
    assert not errors, errors
