"""dct::dct2 and dst::dst4, the direct sums, on device memory over row lengths, HIP events.
In one process a default context (tiled kernel where direct_use_tiled takes it) alternates with a set_direct_tiled(False) context
(simple kernel, one lane per output).  Batches hold about 3e10 terms (at most 64 M input floats); each timed sample runs enough
calls for >= ~5 ms of the slower kernel.  Five rounds after 3 warm-up calls; median [min .. max] ms per call.  Reported per call:
terms / s (batch x n x terms per row), the share of the unfused VALU ceiling (157.3 TFLOP/s counting an FMA as two: a separate
multiply and add per term give 39.3 T terms / s) and the share of HBM (8 bytes per element against 8 TB/s).  The first call of a
fresh context, which builds the n x n table on the host, is timed on the host (first-call ms - steady-state ms = table build).
usage: bench_trig_direct.py [n ...]"""
import sys, pathlib, time; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime

CEIL_TERMS = 157.3e12 / 4  # one mul + one add per term
stream = abtime.one_stream()


def ctx(tiled):
    f = kofft_amd.HipFftImpl(np.float32)
    f.set_direct_tiled(tiled)
    f.set_stream(stream.cuda_stream)
    return f


tiled, simple = ctx(True), ctx(False)
for n in [int(a) for a in sys.argv[1:]] or [32, 64, 256, 1024, 4096]:
    rows = int(min(max(3e10 // (n * n), 64), (64 << 20) // n))
    x = torch.empty((rows, n), dtype=torch.float32, device="cuda").uniform_(-1, 1)
    y = torch.empty_like(x)
    for family, type in (("dct", 2), ("dst", 4)):
        terms = rows * n * (n - 1 if type == 3 else n)
        with torch.cuda.stream(stream):
            fresh = ctx(True)
            t0 = time.perf_counter()
            getattr(fresh, f"{family}_direct_dev")(type, x.data_ptr(), y.data_ptr(), n, rows)
            torch.cuda.synchronize()
            first_ms = (time.perf_counter() - t0) * 1e3
            del fresh
            calls = {"tiled": lambda f=tiled: getattr(f, f"{family}_direct_dev")(type, x.data_ptr(), y.data_ptr(), n, rows),
                     "simple": lambda f=simple: getattr(f, f"{family}_direct_dev")(type, x.data_ptr(), y.data_ptr(), n, rows)}
            for c in calls.values():
                for _ in range(3):
                    c()
            torch.cuda.synchronize()
            one = max(abtime.timed(stream, c, 1) for c in calls.values())
            reps = max(1, min(50, int(5.0 / max(one, 1e-3))))
            times = abtime.alternate(stream, calls, warmup=0, rounds=5, reps=reps)  # (warmed up above)
        line = f"{family}{type} n {n:5d} rows {rows:8d} first-call {first_ms:8.1f} ms:"
        for k, t in times.items():
            md = float(np.median(t))
            tps = terms / (md * 1e-3)
            line += (f" | {k} {abtime.cell(t)} {tps / 1e12:.2f} Tterm/s valu {tps / CEIL_TERMS:.3f}"
                     f" hbm {8 * rows * n / (md * 1e-3) / 8e12:.3f}")
        print(line, flush=True)
    del x, y
    torch.cuda.empty_cache()
