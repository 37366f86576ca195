"""The row-wise families (DCT-II, the analytic signal, the real cepstrum, the direct DCT / DST, the wavelets) on SHARED context state:
the composed routes' scratch (ctx->real_tmp, grown by ensure), the table cache (host_cache.h, TableKind: the twiddle / rfft, Bluestein,
DCT-II and direct kinds), the per-process kernel attributes (set_dyn_lds_once), stream switches, release_scratch, hipGraph
capture, two threads at once and the host pipeline.  Every output is compared bit for bit with the family's oracle, and the host
calls run twice."""
import subprocess
import sys
import textwrap
import threading

import numpy as np
import pytest

import wavelet_oracle as wo
from cepstrum_oracle import cepstrum_ref
from conftest import ROOT, bits_equal, rand_c, seeded
from dct_oracle import dct2_ref
from hilbert_oracle import hilbert_ref
from rowcheck import assert_rows_equal
from trig_direct_oracle import KINDS

pytestmark = pytest.mark.gpu

F = np.float32


def _x(shape, seed):
    return seeded(seed).uniform(-1, 1, shape).astype(F)


def _direct_ref(family, type, x):
    from oracle import pyoracle

    return pyoracle.direct_mt(family, type, x)


def _twice(fn, *args):
    a = fn(*args)
    b = fn(*args)
    pa, pb = (a, b) if isinstance(a, tuple) else ((a,), (b,))
    for u, v in zip(pa, pb):
        us = u if isinstance(u, list) else [u]
        vs = v if isinstance(v, list) else [v]
        assert [np.asarray(p).tobytes() for p in us] == [np.asarray(q).tobytes() for q in vs], f"{fn.__name__}: two runs differ"
    return a


# ---- device-form operations: inputs uploaded up front, outputs read after one synchronisation -----------------------------------

PAD = 4


class Op:
    """One _dev call on fresh device buffers: enqueue(f) on the context's current stream, check() against the oracle afterwards."""

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
                assert_rows_equal(got[o:o + w.size].reshape(w.shape), w, f"{self.what} part {l}")
                o += w.size
        else:
            assert_rows_equal(got.reshape(want.shape), want, self.what)


def op_dct2(n, b, seed):
    x = _x((b, n), seed)
    return Op(f"dct2 n={n} b={b}", [x], b * n, lambda f, i, o: f.dct2_dev(i, o, n, b), lambda: dct2_ref(x))


def op_hilbert(n, b, seed):
    x = _x((b, n), seed)
    return Op(f"hilbert n={n} b={b}", [x], 2 * b * n, lambda f, i, o: f.hilbert_dev(i, o, n, b), lambda: hilbert_ref(x),
              lambda g: g.view(np.complex64).reshape(b, n))


def op_cepstrum(n, b, seed):
    x = _x((b, n), seed)
    return Op(f"cepstrum n={n} b={b}", [x], b * n, lambda f, i, o: f.cepstrum_dev(i, o, n, b), lambda: cepstrum_ref(x))


def op_direct(family, type, n, b, seed):
    x = _x((b, n), seed)
    dev = (lambda f, i, o: f.dct_direct_dev(type, i, o, n, b)) if family == "dct" else (lambda f, i, o: f.dst_direct_dev(type, i, o, n, b))
    return Op(f"{family}{type} n={n} b={b}", [x], b * n, dev, lambda: _direct_ref(family, type, x))


def op_wavedec(name, n, b, levels, seed):
    x = _x((b, n), seed)
    lens = wo.multi_lengths(n, levels)
    na, nd = b * lens[-1], b * sum(lens[1:])

    def call(f, i, o):
        f.wavedec_dev(name, i, o, (o + 4 * na) if levels else 0, n, b, levels)

    def want():
        a, ds = wo.forward_multi(name, x, levels)
        return [a] + ds

    return Op(f"wavedec {name} n={n} b={b} L={levels}", [x], na + nd, call, want)


def op_waverec(name, n0, b, levels, seed):
    ap = _x((b, n0), seed)
    dl = [n0 << (levels - 1 - l) for l in range(levels)]
    dets = [_x((b, m), seed + 1 + l) for l, m in enumerate(dl)]
    packed = np.concatenate([d.ravel() for d in dets]) if dets else np.zeros(1, F)

    def call(f, a, d, o):
        f.waverec_dev(name, a, d, dl, o, n0, b)

    return Op(f"waverec {name} n0={n0} b={b} L={levels}", [ap, packed], b * (n0 << levels), call,
              lambda: wo.inverse_multi(name, ap, dets))


def _streams():
    import torch

    return torch.cuda.Stream(), torch.cuda.Stream()


# ---- 1. stream switching over the shared scratch ----------------------------------------------------------------------------------

def test_stream_switching_over_real_tmp(oracle):
    """Composed dct2 (n = 1000: not a power of two), composed cepstrum (n = 8192), per-level wavedec / waverec (levels > 1) on one
    context, alternating two streams with no host synchronisation: every call uses ctx->real_tmp, and the sizes are ordered so that it
    must grow (free + allocate) in the middle of the sequence, while work on the other stream may still read the old buffer."""
    import torch

    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    f.set_wavelet_fused(0)
    s1, s2 = _streams()
    ops = [op_dct2(1000, 4, 100), op_cepstrum(8192, 2, 101), op_wavedec("db4", 3000, 8, 3, 102), op_waverec("sym4", 375, 8, 3, 103),
           op_dct2(1000, 300, 104), op_cepstrum(8192, 40, 105), op_wavedec("coif1", 20000, 40, 4, 106),
           op_waverec("db2", 1250, 40, 4, 107), op_dct2(999, 8, 108), op_cepstrum(16384, 3, 109)]
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
    """The first dct2 and direct call of a size (tables built and uploaded) on s1, the next call of that size on s2 without a sync."""
    import torch

    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    s1, s2 = _streams()
    pairs = [(op_dct2(3000, 64, 200), op_dct2(3000, 64, 201)), (op_dct2(2048, 70, 202), op_dct2(2048, 70, 203)),
             (op_direct("dct", 3, 700, 129, 204), op_direct("dct", 3, 700, 129, 205)),
             (op_direct("dst", 1, 130, 5, 206), op_direct("dst", 1, 130, 5, 207))]
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
    """release_scratch between a composed call of one family and a composed call of another, and after a fused call: unchanged output."""
    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    f.set_cepstrum_fused(False)
    f.set_wavelet_fused(0)
    x1, x2, x3 = _x((50, 1000), 300), _x((9, 4096), 301), _x((17, 1024), 302)
    w1, w2, w3 = dct2_ref(x1), cepstrum_ref(x2), hilbert_ref(x3)
    wa, wds = wo.forward_multi("sym4", x2, 3)
    for rep in range(2):
        assert_rows_equal(_twice(f.dct2_batch, x1), w1, "composed dct2")
        f.release_scratch()
        assert_rows_equal(_twice(f.cepstrum_batch, x2), w2, "composed cepstrum")
        f.release_scratch()
        assert_rows_equal(_twice(f.hilbert_batch, x3), w3, "fused hilbert")
        f.release_scratch()
        a, ds = _twice(f.wavedec_batch, x2, "sym4", 3)
        assert_rows_equal(a, wa, "per-level wavedec")
        for g, w in zip(ds, wds):
            assert_rows_equal(g, w, "per-level wavedec detail")
        f.release_scratch()
    f.close()


# ---- 4. every family interleaved with the core users of real_tmp -------------------------------------------------------------------

def test_families_interleaved_with_core_users_on_one_context(oracle):
    """One context: the row-wise families between a composed non-power-of-two rfft, an STFT with a non-power-of-two window and fftnd,
    sizes growing and shrinking; n = 1000 reused across kinds (twiddle / rfft, Bluestein, DCT-II, all eight direct kinds, wavelets).
    fftnd has no CPU oracle here: it must give the bytes of a fresh context."""
    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    fresh = kofft_amd.HipFftImpl(np.float32)
    rng = seeded(400)
    nd = rand_c(rng, (2 * 96 * 1000,))
    nd_want = nd.copy()
    fresh.fftnd(nd_want, 2, 96, 1000)
    sig = rng.uniform(-1, 1, 30000).astype(F)
    win = rng.uniform(0.1, 1, 1000).astype(F)
    frames = -(-sig.size // 250)
    for rep, (b_small, b_big) in enumerate([(3, 200), (150, 7), (2, 40)]):
        xr = _x((b_big, 3000), 410 + rep)
        assert bits_equal(f.rfft_batch(xr), oracle.rfft(xr, None)), "composed rfft n=3000"
        x = _x((b_small, 1000), 420 + rep)
        assert_rows_equal(_twice(f.dct2_batch, x), dct2_ref(x), "dct2 n=1000")
        for family, type in KINDS:
            got = _twice(f.dct_direct_batch if family == "dct" else f.dst_direct_batch, x, type)
            assert_rows_equal(got, _direct_ref(family, type, x), f"{family}{type} n=1000")
        xc = rand_c(rng, (b_big, 1000))
        y = xc.copy()
        f.fft_batch(y)
        assert bits_equal(y, oracle.fft(xc)), "Bluestein n=1000"
        assert bits_equal(f.stft_into(sig, win, 250, frames), oracle.stft(sig, win, 250, frames)), "stft win=1000"
        xw = _x((b_big, 1000), 430 + rep)
        a, ds = _twice(f.wavedec_batch, xw, "db4", 4)
        wa, wds = wo.forward_multi("db4", xw, 4)
        assert_rows_equal(a, wa, "wavedec n=1000")
        for g, w in zip(ds, wds):
            assert_rows_equal(g, w, "wavedec detail n=1000")
        xp = _x((b_small, 1 << (10 + 3 * rep)), 440 + rep)
        assert_rows_equal(_twice(f.cepstrum_batch, xp), cepstrum_ref(xp), "cepstrum")
        assert_rows_equal(_twice(f.hilbert_batch, xp), hilbert_ref(xp), "hilbert")
        z = nd.copy()
        f.fftnd(z, 2, 96, 1000)
        assert bits_equal(z, nd_want), "fftnd 2 x 96 x 1000"
    f.close()
    fresh.close()


# ---- 5. hipGraph capture -------------------------------------------------------------------------------------------------------

def test_rowwise_device_calls_can_be_captured_into_a_hip_graph(oracle):
    """After a warm-up (tables uploaded, scratch grown, kernel attributes set) every family's _dev calls are kernel launches and
    device copies on the context's stream: captured in sequence on one side stream -- fused and composed dct2 / hilbert / cepstrum,
    tiled and simple direct, fused and per-level wavedec / waverec and levels == 0 -- nothing runs before replay, and two replays give
    the direct calls' bytes, which are the oracle's."""
    import torch

    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    s = torch.cuda.Stream()
    f.set_stream(s.cuda_stream)
    # (route, op): route set on the context right before the call -- a host-side switch, read at enqueue time
    plan = [
        ("dct_fused", op_dct2(1024, 9, 500)), ("dct_composed", op_dct2(1000, 9, 501)),
        ("hilbert_fused", op_hilbert(1024, 5, 502)), ("hilbert_composed", op_hilbert(1024, 5, 503)),
        ("cepstrum_fused", op_cepstrum(2048, 5, 504)), ("cepstrum_composed", op_cepstrum(2048, 5, 505)),
        ("tiled", op_direct("dct", 2, 256, 128, 506)), ("simple", op_direct("dst", 4, 256, 128, 507)),
        ("wav_fused", op_wavedec("db4", 4096, 6, 4, 508)), ("wav_perlevel", op_wavedec("db4", 4096, 6, 4, 509)),
        ("wav_fused", op_waverec("coif1", 256, 6, 4, 510)), ("wav_perlevel", op_waverec("coif1", 256, 6, 4, 511)),
        ("wav_fused", op_wavedec("haar", 777, 3, 0, 512)), ("wav_fused", op_waverec("haar", 777, 3, 0, 513)),
    ]

    def route(r):
        f.set_dct_fused(r != "dct_composed")
        f.set_hilbert_fused(r != "hilbert_composed")
        f.set_cepstrum_fused(r != "cepstrum_composed")
        f.set_direct_tiled(r != "simple")
        f.set_wavelet_fused(0 if r == "wav_perlevel" else 2)

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
    """One thread builds direct tables at n = 4096 (the 16-thread host build) while the other makes first-use dct2 / hilbert /
    cepstrum calls at sizes no other context of this test has seen; both run fused wavelet calls whose LDS exceeds 64 KiB (lengths
    12000 and 16384: different sizes on the same kernel instance, whose LDS attribute is set once per process).  Every result must be
    the oracle's.  A worker that fails before the barrier breaks it, so the other one cannot wait forever."""
    import kofft_amd

    errors = []
    barrier = threading.Barrier(2, timeout=120)

    def fused_wavelet(f, n, seed):
        x = _x((3, n), seed)
        a, ds = f.wavedec_batch(x, "sym4", 3)
        wa, wds = wo.forward_multi("sym4", x, 3)
        assert_rows_equal(a, wa, f"fused wavedec n={n}")
        for g, w in zip(ds, wds):
            assert_rows_equal(g, w, f"fused wavedec n={n} detail")

    def direct_worker():
        try:
            f = kofft_amd.HipFftImpl(np.float32)
            f.set_wavelet_fused(2)
            barrier.wait()
            x = _x((3, 4096), 600)
            for family, type in (("dct", 2), ("dst", 3), ("dct", 4)):
                got = _twice(f.dct_direct_batch if family == "dct" else f.dst_direct_batch, x, type)
                assert_rows_equal(got, _direct_ref(family, type, x), f"{family}{type} n=4096")
            fused_wavelet(f, 16384, 601)
            fused_wavelet(f, 12000, 602)
            f.close()
        except Exception as e:  # noqa: BLE001 -- reported below, in the main thread
            barrier.abort()
            errors.append(repr(e))

    def fft_worker():
        try:
            f = kofft_amd.HipFftImpl(np.float32)
            f.set_wavelet_fused(2)
            barrier.wait()
            fused_wavelet(f, 12000, 610)
            for n, b in ((2048 * 3, 5), (1 << 13, 9), (512, 300)):
                x = _x((b, n), 611 + n)
                assert_rows_equal(_twice(f.dct2_batch, x), dct2_ref(x), f"dct2 n={n}")
                if n & (n - 1) == 0:
                    assert_rows_equal(_twice(f.hilbert_batch, x), hilbert_ref(x), f"hilbert n={n}")
                    assert_rows_equal(_twice(f.cepstrum_batch, x), cepstrum_ref(x), f"cepstrum n={n}")
            fused_wavelet(f, 16384, 612)
            f.close()
        except Exception as e:  # noqa: BLE001
            barrier.abort()
            errors.append(repr(e))

    a, b = threading.Thread(target=direct_worker, daemon=True), threading.Thread(target=fft_worker, daemon=True)
    a.start(); b.start(); a.join(300); b.join(300)
    assert not (a.is_alive() or b.is_alive()), "a worker did not finish within 300 s"
    assert not errors, errors


def test_fused_wavelet_lds_attribute_in_a_fresh_process():
    """The fused forward wavelet kernel's dynamic LDS depends on the row length (6 bytes per sample from 8192 on: 72000 at 12000, 98304
    at 16384), and its LDS attribute is set once per process (to the kernel's largest).  In a fresh process, so that no
    earlier test has set it, a first call at 12000 is followed by longer and shorter rows: every result must be the oracle's.  This
    checks the results of that order only: the ROCm runtime here does not reject a launch whose LDS exceeds the value set, so the value
    itself is not observable."""
    script = textwrap.dedent("""
        import sys
        import numpy as np
        sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
        import kofft_amd, wavelet_oracle as wo
        f = kofft_amd.HipFftImpl(np.float32)
        f.set_wavelet_fused(2)
        for n in (12000, 16384, 10924, 16000):
            x = np.random.default_rng(n).uniform(-1, 1, (2, n)).astype(np.float32)
            a, ds = f.wavedec_batch(x, "db2", 2)
            wa, wds = wo.forward_multi("db2", x, 2)
            assert a.tobytes() == wa.tobytes() and all(g.tobytes() == w.tobytes() for g, w in zip(ds, wds)), n
        print("ok")
    """)
    res = subprocess.run([sys.executable, "-c", script, str(ROOT)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "ok" in res.stdout, res.stdout + res.stderr


# ---- 7. the host pipeline ON -----------------------------------------------------------------------------------------------------

def test_host_pipeline_on_rowwise_forms(oracle, monkeypatch):
    """KOFFT_HIP_HOST_PIPELINE=1 (the shipped default for 128 MiB and more): hilbert with its complex output and the multi-level
    wavedec / waverec host forms (which do not pipeline: packed details) at batches that do not divide by 8, against the pipeline OFF
    and the oracle; direct_host bypasses the pipeline, and in == out still gives the oracle's bytes at that size."""
    import kofft_amd

    xh = _x((4100 + 3, 4096), 700)             # 67 MB in, 134 MB out
    xw = _x((517, 1 << 16), 701)               # 135 MB in
    ap = _x((523, 8192), 702)                  # 8192 << 3 = 65536 out per row: 137 MB
    dets = [_x((523, 8192 << (2 - l)), 703 + l) for l in range(3)]
    xd = _x(((1 << 19) + 3, 64), 710)          # 134 MB, in place
    outs = []
    for pipe in ("1", "0"):
        monkeypatch.setenv("KOFFT_HIP_HOST_PIPELINE", pipe)  # read when the context is created
        f = kofft_amd.HipFftImpl(np.float32)
        h = _twice(f.hilbert_batch, xh)
        a, ds = _twice(f.wavedec_batch, xw, "db4", 3)
        r = _twice(f.waverec_batch, ap, dets, "db2")
        buf = xd.copy()
        f._check(f._lib.kofft_hip_dst_direct_f32(f._ctx, 2, buf.ctypes.data, buf.ctypes.data, 64, buf.shape[0]))
        outs.append((h, a, ds, r, buf))
        f.close()
    (h, a, ds, r, buf), off = outs
    assert h.tobytes() == off[0].tobytes() and a.tobytes() == off[1].tobytes() and r.tobytes() == off[3].tobytes()
    assert [d.tobytes() for d in ds] == [d.tobytes() for d in off[2]] and buf.tobytes() == off[4].tobytes()
    assert_rows_equal(h, hilbert_ref(xh), "pipelined hilbert")
    wa, wds = wo.forward_multi("db4", xw, 3)
    assert_rows_equal(a, wa, "wavedec")
    for g, w in zip(ds, wds):
        assert_rows_equal(g, w, "wavedec detail")
    assert_rows_equal(r, wo.inverse_multi("db2", ap, dets), "waverec")
    assert_rows_equal(buf, _direct_ref("dst", 2, xd), "dst2 in place")
