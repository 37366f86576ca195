"""The spectral families (planar fft_split, chirp-Z, Goertzel, the Hartley transform, the polyphase filter bank) on SHARED context
state: the composed routes' scratch (ctx->real_tmp for the packed planar rows, the folded analysis frames and the
completed synthesis frames; ctx->rows_tmp for the synthesis' real frames, both routes), the chirp-Z table slots (a 4-entry LRU that
release_scratch drops), the Goertzel coefficient set of the device form, the Hartley tables (kept until destroy) and the direct
kernels under their shared switch, stream switches, release_scratch, hipGraph capture and two threads at once.  The tests mirror those of
tests/test_gpu_filter_context.py; every output is compared bit for bit with the family's oracle, and the host calls run twice."""
import threading

import numpy as np
import pytest

import hartley_oracle as ho
import mdct_oracle as mo
import pfb_oracle as po
import spectral_oracle as so
from conftest import bits_equal, seeded
from convolve_oracle import convolve_ref
from rowcheck import assert_rows_equal
from split_oracle import split_ref

pytestmark = pytest.mark.gpu

F = np.float32
PAD = 4
KNOB = "KOFFT_HIP_SCRATCH_CHUNK_MB"
RATE = 8000.0


def _x(shape, seed):
    return seeded(seed).uniform(-1, 1, shape).astype(F)


def _spec(shape, seed):
    rng = seeded(seed)
    return (rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)).astype(np.complex64)


def _wa(m, name):
    return so.param_sets(m)[name]


def _twice(fn, *args, **kw):
    a = fn(*args, **kw)
    b = fn(*args, **kw)
    pa, pb = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    for u, v in zip(pa, pb):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes(), f"{fn.__name__}: two runs differ"
    return a


def _rows(a):
    """[rows, floats]: the bits of a real or complex array, its last axis a row"""
    a = np.ascontiguousarray(a)
    return a.reshape(-1, a.shape[-1]).view(F)


def _same(got, want, what):
    assert_rows_equal(_rows(got), _rows(want), what)


def _split_host(f, re, im, inverse=False):
    r, i = re.copy(), im.copy()
    f.fft_split_batch(r, i, inverse)
    return r, i


# ---- device-form operations: inputs uploaded up front, outputs read after one synchronisation -----------------------------------
class Op:
    """One _dev call on fresh device buffers: enqueue(f) on the context's current stream, check() against the oracle afterwards.
    `want()` is a list of arrays (real or complex) that lie one behind the other in the output buffer."""

    def __init__(self, what, inputs, out_floats, call, want):
        import torch

        self.what = what
        self.ins = [torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(F).copy()).cuda() for a in inputs]
        self.out = torch.full((out_floats + PAD,), 7.0, dtype=torch.float32, device="cuda")  # PAD floats behind the output: checked by result()
        self.out_floats, self.fill = out_floats, 7.0
        self.call, self.want = call, want

    def enqueue(self, f):
        self.call(f, *[t.data_ptr() for t in self.ins], self.out.data_ptr())

    def result(self):
        assert bool((self.out[self.out_floats:] == self.fill).all()), f"{self.what}: the padding behind the output was written"
        return self.out[:self.out_floats].cpu().numpy()

    def check(self):
        got = self.result()
        o = 0
        for l, w in enumerate(self.want()):
            w = _rows(w)
            assert_rows_equal(got[o:o + w.size].reshape(w.shape), w, f"{self.what} part {l}")
            o += w.size
        assert o == self.out_floats, (self.what, o, self.out_floats)


def op_split(n, b, seed, inverse=False, fused=False):
    re, im = _x((b, n), seed), _x((b, n), seed + 1)

    def call(f, dre, dim, o):
        f.set_split_fused(fused)
        rc = f._lib.kofft_hip_dev_fft_split_c32(f._ctx, dre, dim, o, o + 4 * b * n, n, b, int(inverse))
        assert rc == 0, rc

    return Op(f"fft_split n={n} b={b} inverse={inverse} fused={fused}", [re, im], 2 * b * n, call, lambda: list(split_ref(re, im, inverse)))


def op_czt(n, m, name, b, seed, route=0):
    x = _x((b, n), seed)
    w, a = _wa(m, name)

    def call(f, dx, o):
        f.set_czt_route(route)
        f.czt_dev(dx, o, n, m, w, a, b)

    return Op(f"czt n={n} m={m} {name} b={b} route={route}", [x], 2 * b * m, call, lambda: [so.czt(x, m, w, a)])


def op_goertzel(n, b, freqs, seed):
    x = _x((b, n), seed)
    freqs = np.asarray(freqs, F)
    return Op(f"goertzel n={n} b={b} nfreq={freqs.size}", [x], b * freqs.size, lambda f, dx, o: f.goertzel_dev(dx, o, n, b, RATE, freqs),
              lambda: [so.goertzel(x, RATE, freqs).reshape(b, freqs.size)])


def op_dht(n, b, seed, tiled=True):
    x = _x((b, n), seed)

    def call(f, dx, o):
        f.set_direct_tiled(tiled)
        f.dht_dev(dx, o, n, b)

    return Op(f"dht n={n} b={b} tiled={tiled}", [x], b * n, call, lambda: [ho.dht(x)])


def op_analysis(m, taps, hop, lead, rows, nx, bins, seed, route=0):
    x, h = _x((rows, nx), seed), _x((taps * m,), seed + 1)
    frames = -(-(nx + lead) // hop) + 1

    def call(f, dx, dh, o):
        f.set_pfb_fused(route)
        f.pfb_analysis_dev(dx, rows, nx, nx, dh, taps * m, m, hop, lead, o, frames, bins)

    return Op(f"pfb_analysis M={m} T={taps} D={hop} lead={lead} rows={rows} nx={nx} bins={bins} route={route}", [x, h], 2 * rows * frames * bins, call,
              lambda: [po.analysis_ref(x, h, m, hop, lead, frames, bins)])


def op_synthesis(m, taps, hop, rows, frames, bins, seed, route=0, scale=0.37, first=0, count=None):
    S, g = _spec((rows, frames, bins), seed), _x((taps * m,), seed + 1)
    full = (frames - 1) * hop + taps * m
    count = full - first if count is None else count

    def call(f, ds, dg, o):
        f.set_pfb_fused(route)
        f.pfb_synthesis_dev(ds, rows, frames, bins, dg, taps * m, m, hop, scale, o, first, count)

    return Op(f"pfb_synthesis M={m} T={taps} D={hop} rows={rows} frames={frames} bins={bins} route={route} window={first}+{count}", [S, g],
              rows * count, call, lambda: [po.synthesis_ref(S, g, m, hop, scale)[:, first:first + count]])


def _streams():
    import torch

    return torch.cuda.Stream(), torch.cuda.Stream()


def _reset(f):
    f.set_split_fused(True)
    f.set_czt_route(0)
    f.set_direct_tiled(True)
    f.set_pfb_fused(1)
    f.set_stream(0)


# ---- 1. stream switching over the shared scratch ----------------------------------------------------------------------------------
def test_stream_switching_over_real_tmp_and_rows_tmp(oracle):
    """The composed split (its packed rows in real_tmp), the composed analysis (its folded frames there), the composed synthesis (its
    completed frames there, their real parts in rows_tmp) and the fused synthesis (rows_tmp alone) on one context, alternating two
    streams with no host synchronisation.  The sizes are ordered so that real_tmp must grow at the second split (2.3 MiB after 12 KiB),
    again at the M = 16384 analysis (3.9 MiB) and again at the large composed synthesis (4.2 MiB), and rows_tmp at the large fused
    synthesis (1.6 MiB after 3 KiB) and again at the large composed one (2.1 MiB), while work on the other stream may still read the
    old buffer; then they shrink again.  Two passes: every op equals the oracle and its own first pass."""
    import torch

    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    s1, s2 = _streams()
    ops = [op_split(12, 5, 100), op_analysis(240, 2, 100, 0, 2, 1500, 121, 102), op_synthesis(64, 3, 24, 2, 6, 33, 104),
           op_synthesis(64, 3, 24, 2, 6, 64, 106, route=2), op_split(1000, 300, 108, inverse=True), op_analysis(16384, 2, 8192, 16384, 3, 60000, 16384, 110),
           op_synthesis(1024, 4, 256, 4, 100, 513, 112, route=1), op_synthesis(2048, 2, 1000, 3, 85, 2048, 114, first=777, count=50000),
           op_split(15, 33, 116), op_analysis(6, 3, 7, 5, 3, 200, 4, 118), op_synthesis(240, 1, 120, 2, 9, 121, 120), op_split(4097, 9, 122),
           op_synthesis(32, 8, 1, 3, 40, 17, 124, route=2)]
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
    _reset(f)
    f.close()


# ---- 2. state built on one stream, used on another -----------------------------------------------------------------------------------
def test_state_built_on_one_stream_used_on_another(oracle):
    """The first table-route chirp-Z of a key (its table built by a kernel), the first dht of a length (its table built by a kernel, or
    on the host and uploaded) and the first Goertzel call of a coefficient set (brought over by a kernel) on s1; the next call with the
    same key, length or coefficient bits -- which builds and uploads nothing -- on s2 without a sync."""
    import torch

    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    s1, s2 = _streams()
    freqs = seeded(200).uniform(0, RATE / 2, 300)
    pairs = [(op_czt(256, 64, "zoom", 9, 201, route=2), op_czt(256, 64, "zoom", 70, 202, route=0)),
             (op_dht(1000, 5, 203), op_dht(1000, 70, 204)),
             (op_goertzel(1000, 3, freqs, 205), op_goertzel(1000, 5, freqs, 206)),
             (op_czt(1000, 255, "dft", 2, 207, route=1), op_czt(1000, 255, "dft", 3, 208, route=2)),
             (op_goertzel(1000, 2, freqs[:7], 209), op_goertzel(1000, 4, freqs[:7], 210))]
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(pairs):
        f.set_dht_table_device(k % 2 == 1)
        f.set_stream(s1.cuda_stream)
        a.enqueue(f)
        f.set_stream(s2.cuda_stream)
        b.enqueue(f)
    torch.cuda.synchronize()
    for a, b in pairs:
        a.check()
        b.check()
    _reset(f)
    f.close()


# ---- 3. release_scratch between families ------------------------------------------------------------------------------------------
def test_release_scratch_between_families(oracle):
    """release_scratch between the families: the chirp-Z key is rebuilt (its slot and table went with the release) and gives the same
    bytes; the Goertzel device call with the coefficient bits of before the release is still right (the coefficients went too, so the
    bits must not be taken for uploaded); the dht of a length seen before is still right (its table survives the release); the composed
    split, analysis and synthesis get their scratch anew."""
    import torch

    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    freqs = seeded(300).uniform(0, RATE / 2, 257)
    ops = [op_czt(257, 65, "zoom", 9, 301, route=2), op_goertzel(1023, 5, freqs, 302), op_dht(257, 70, 303), op_split(1000, 7, 304),
           op_analysis(240, 3, 77, 100, 2, 2000, 240, 305), op_synthesis(240, 3, 77, 2, 11, 121, 306), op_czt(257, 65, "zoom", 3, 307, route=0)]
    first = None
    for rep in range(3):
        for op in ops:
            op.out.fill_(7.0)
            torch.cuda.synchronize()
            op.enqueue(f)
            f.synchronize()
            op.check()
            f.release_scratch()
        now = [op.result().tobytes() for op in ops]
        assert first is None or now == first, "a pass after release_scratch differs from the first"
        first = now
    _reset(f)
    f.close()


# ---- 4. every family interleaved with the older users of the same scratch -------------------------------------------------------------
def test_families_interleaved_with_older_users_of_the_scratch(oracle):
    """One context under a 1 MiB scratch chunk: the families between a composed rfft (n = 3000), an STFT with a 1000-point window, the
    overlap-save convolve, a direct DCT of the dht's length (the same kernels and switch) and an MDCT, sizes growing and shrinking over
    three rounds and the routes alternating."""
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
    hv = _x((100,), 401)
    freqs = rng.uniform(0, RATE / 2, 40).astype(F)
    for rep, (b_small, b_big) in enumerate([(3, 200), (150, 7), (2, 70)]):
        f.set_split_fused(rep % 2 == 1)
        f.set_pfb_fused(rep % 3)
        f.set_direct_tiled(rep % 2 == 0)
        f.set_czt_route([0, 2, 1][rep])
        xr = _x((b_big, 3000), 410 + rep)
        assert bits_equal(f.rfft_batch(xr), oracle.rfft(xr, None)), "composed rfft n=3000"
        re, im = _x((b_big, 1000), 420 + rep), _x((b_big, 1000), 425 + rep)
        gr, gi = _twice(_split_host, f, re, im, bool(rep % 2))
        wr, wi = split_ref(re, im, bool(rep % 2))
        _same(gr, wr, "fft_split n=1000 re")
        _same(gi, wi, "fft_split n=1000 im")
        assert bits_equal(f.stft_into(sig, win, 250, frames), oracle.stft(sig, win, 250, frames)), "stft win=1000"
        xa, ha = _x((b_small, 3000), 430 + rep), _x((2 * 512,), 435 + rep)
        fa = -(-(3000 + 512) // 200) + 1
        _same(_twice(f.pfb_analysis, xa, ha, 512, 200, 512, fa, 257), po.analysis_ref(xa, ha, 512, 200, 512, fa, 257), "pfb analysis M=512")
        xd = _x((b_big, 256), 440 + rep)
        _same(_twice(f.dht_batch, xd), ho.dht(xd), "dht n=256")
        _same(_twice(f.dct_direct_batch, xd, 2), oracle.direct_mt("dct", 2, xd), "direct DCT-II n=256")
        xv = _x((min(b_small, 17), 20000), 450 + rep)
        _same(_twice(f.convolve_rows, xv, hv, block=1024), convolve_ref(xv, hv, 1024), "overlap-save convolve")
        Ss, gs = _spec((b_small, 20, 1024), 460 + rep), _x((4 * 1024,), 465 + rep)
        _same(_twice(f.pfb_synthesis, Ss, gs, 1024, 300, 0.5), po.synthesis_ref(Ss, gs, 1024, 300, 0.5), "pfb synthesis M=1024")
        xc = _x((b_big, 255), 470 + rep)
        w, a = _wa(100, "zoom")
        _same(_twice(f.czt, xc, 100, w, a), so.czt(xc, 100, w, a), "czt n=255 m=100")
        xm, wm = _x((b_small, 5000), 480 + rep), seeded(485 + rep).uniform(0.1, 1.0, 2 * 960).astype(F)
        got = _twice(f.mdct_rows, xm, wm)
        _same(got, mo.mdct_ref(xm, wm, 960, -(-5000 // 960) + 1), "mdct N=960")
        xg = _x((b_big, 1000), 490 + rep)
        _same(_twice(f.goertzel, xg, RATE, freqs), so.goertzel(xg, RATE, freqs), "goertzel n=1000")
    _reset(f)
    f.close()


# ---- 5. a chirp-Z churn under the default route -----------------------------------------------------------------------------------------
def test_five_key_czt_churn_with_dht_and_goertzel_in_between(oracle):
    """Five chirp-Z keys through the four slots with the route at 0 throughout, so that whether a call sums on the fly or through a
    table depends on the batch and on what the calls before left (a fresh table from batch 8, a cached one from batch 2), and every
    fifth use finds its key evicted; dht and Goertzel device calls in between run on the direct kernels and the coefficient buffer the
    chirp-Z shares the context with.  Every result is the oracle's, whichever route the state picked, and the same on a second run
    (whose state differs: the first run may have built the table)."""
    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    keys = [(256, 64, "zoom"), (255, 100, "dft"), (1000, 33, "zoom"), (64, 257, "a_zero"), (257, 256, "dft")]
    batches = [1, 2, 9, 3, 8, 70, 2, 1, 12, 2, 64, 7, 2, 9, 1, 3]
    order = [0, 1, 2, 3, 4, 0, 0, 1, 2, 2, 3, 4, 0, 1, 1, 2]   # (0 1 2 3 4 0: the first key comes back after its eviction)
    freqs = seeded(500).uniform(0, RATE / 2, 9).astype(F)
    for k, (ki, b) in enumerate(zip(order, batches)):
        n, m, name = keys[ki]
        x = _x((b, n), 510 + k)
        w, a = _wa(m, name)
        _same(_twice(f.czt, x, m, w, a), so.czt(x, m, w, a), f"czt churn step {k}: n={n} m={m} {name} batch={b}")
        if k % 3 == 1:
            xd = _x((66, n), 530 + k)
            _same(_twice(f.dht_batch, xd), ho.dht(xd), f"dht n={n} after churn step {k}")
        if k % 3 == 2:
            xg = _x((5, n), 550 + k)
            _same(_twice(f.goertzel, xg, RATE, freqs[:1 + k % 9]), so.goertzel(xg, RATE, freqs[:1 + k % 9]).reshape(5, -1), f"goertzel after churn step {k}")
    f.close()


# ---- 6. hipGraph capture -------------------------------------------------------------------------------------------------------
def test_spectral_device_calls_can_be_captured_into_a_hip_graph(oracle):
    """After a warm-up (tables built, slots taken, scratch grown) every family's _dev call is kernel launches on the context's stream
    and nothing else: ensure() returns at once when the buffer is large enough, a chirp-Z key among the four of the plan is one find,
    a Hartley table is one find, and a Goertzel coefficient set goes over in a kernel's arguments.  Captured in sequence on one side
    stream (a linear graph) -- both split routes, the three chirp-Z routes, Goertzel with two sets, both direct kernels under the dht,
    and the analysis and the synthesis on their fused and composed routes -- nothing runs before replay, and two replays give the
    direct calls' bytes, which are the oracle's."""
    import torch

    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    s = torch.cuda.Stream()
    f.set_stream(s.cuda_stream)
    freqs = seeded(600).uniform(0, RATE / 2, 300)
    plan = [op_split(1024, 5, 601, fused=True), op_split(1024, 5, 603, fused=False), op_split(1000, 4, 605, inverse=True),
            op_czt(256, 64, "zoom", 9, 607, route=1), op_czt(256, 64, "zoom", 9, 608, route=2), op_czt(256, 64, "zoom", 9, 609, route=0),
            op_czt(63, 257, "dft", 70, 610, route=2), op_czt(0, 5, "dft", 3, 611, route=0),
            op_goertzel(1000, 5, freqs, 612), op_goertzel(1000, 5, freqs[:7], 613), op_goertzel(1023, 70, freqs[:7], 614),
            op_dht(256, 70, 615, tiled=True), op_dht(256, 70, 616, tiled=False), op_dht(17, 3, 617),
            op_analysis(256, 3, 100, 50, 3, 2000, 129, 618, route=1), op_analysis(256, 3, 100, 50, 3, 2000, 129, 620, route=0),
            op_analysis(240, 2, 240, 0, 2, 1500, 240, 622, route=2),
            op_synthesis(256, 3, 100, 3, 12, 129, 624, route=1), op_synthesis(256, 3, 100, 3, 12, 129, 626, route=0),
            op_synthesis(240, 2, 300, 2, 7, 240, 628, route=2, first=5, count=900)]
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for op in plan:  # warm-up, outside the capture: each call's (size, key) once, so that the capture allocates, uploads and evicts nothing
            op.enqueue(f)
    torch.cuda.synchronize()
    direct_bytes = [op.result().tobytes() for op in plan]
    for op in plan:
        op.out.fill_(0.0)
        op.fill = 0.0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for op in plan:
            op.enqueue(f)
    torch.cuda.synchronize()
    for op in plan:
        assert float(op.out.abs().sum()) == 0.0, f"{op.what}: ran during the capture"
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    for op, b in zip(plan, direct_bytes):
        assert op.result().tobytes() == b, f"{op.what}: the replay differs from the direct call"
        op.check()
    _reset(f)
    f.close()


# ---- 7. two threads, fresh contexts, first uses at the same time --------------------------------------------------------------
def test_two_threads_first_uses_at_the_same_time(oracle):
    """Two threads, each on a fresh context, make their first dht of the same length and their first chirp-Z of the same key at the
    same time (the tables are built twice, once per context), then first uses of the other families.  Every result
    must be the oracle's.  A worker that fails before the barrier breaks it, so the other one cannot wait forever."""
    import kofft_amd

    errors = []
    barrier = threading.Barrier(2, timeout=120)
    freqs = seeded(700).uniform(0, RATE / 2, 33).astype(F)
    w, a = _wa(64, "zoom")

    def steps(f, k):
        def dht():
            x = _x((70, 1000), 710 + k)
            _same(_twice(f.dht_batch, x), ho.dht(x), "dht n=1000")

        def czt():
            f.set_czt_route(2)
            x = _x((9, 256), 720 + k)
            _same(_twice(f.czt, x, 64, w, a), so.czt(x, 64, w, a), "czt n=256 m=64")

        def rest():
            x = _x((5, 1000), 730 + k)
            _same(_twice(f.goertzel, x, RATE, freqs), so.goertzel(x, RATE, freqs), "goertzel")
            re, im = _x((7, 1000), 740 + k), _x((7, 1000), 745 + k)
            gr, gi = _twice(_split_host, f, re, im)
            wr, wi = split_ref(re, im)
            _same(gr, wr, "fft_split re")
            _same(gi, wi, "fft_split im")
            xa, ha = _x((3, 3000), 750 + k), _x((3 * 240,), 755 + k)
            Z = _twice(f.pfb_analysis, xa, ha, 240, 100, 0, 31, 240)
            want = po.analysis_ref(xa, ha, 240, 100, 0, 31, 240)
            _same(Z, want, "pfb analysis M=240")
            _same(_twice(f.pfb_synthesis, want, ha, 240, 100, 0.5), po.synthesis_ref(want, ha, 240, 100, 0.5), "pfb synthesis M=240")

        return [dht, czt, rest]

    def worker(k):
        try:
            f = kofft_amd.HipFftImpl(np.float32)
            order = steps(f, k)
            barrier.wait()
            for step in order:
                step()
            f.close()
        except Exception as e:  # noqa: BLE001 -- reported below, in the main thread
            barrier.abort()
            errors.append(repr(e))

    t = [threading.Thread(target=worker, args=(k,), daemon=True) for k in range(2)]
    for th in t:
        th.start()
    for th in t:
        th.join(300)
    assert not any(th.is_alive() for th in t), "a worker did not finish within 300 s"
    assert not errors, errors
