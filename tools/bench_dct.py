"""DctPlanner::plan_dct2 (dct.rs:61-105) on device memory over row lengths: ~1 GiB of input rows per call, HIP events.
In one process a default context (fused kernel for powers of two 32 .. 4096) alternates with a set_dct_fused(False) context
(mirror kernel -> n-point transform -> post-pass kernel), and, for scale, the library's rfft of the same rows already mirrored to
2n reals (what a caller ran on the device without this entry point, before its own mirror and twist).  Five rounds of 10 timed
calls each, after 3 warm-up calls; median [min .. max] ms per call.  Fraction of the roofline: 8 TB/s on 8n bytes per row.
usage: bench_dct.py [n ...]"""
import sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime
fused = kofft_amd.HipFftImpl(np.float32)
composed = kofft_amd.HipFftImpl(np.float32)
composed.set_dct_fused(False)
stream = abtime.one_stream(fused, composed)


for n in [int(a) for a in sys.argv[1:]] or [8, 64, 256, 1024, 4096, 16384, 65536]:
    rows = (1 << 28) // n
    x = torch.empty((rows, n), dtype=torch.float32, device="cuda").uniform_(-1, 1)
    y = torch.empty_like(x)
    mirrored = torch.cat([x, x.flip(1)], dim=1)
    spec = torch.empty((rows, n + 1), dtype=torch.complex64, device="cuda")
    calls = {"fused": lambda: fused.dct2_dev(x.data_ptr(), y.data_ptr(), n, rows),
             "composed": lambda: composed.dct2_dev(x.data_ptr(), y.data_ptr(), n, rows),
             "rfft": lambda: fused.rfft_dev(mirrored.data_ptr(), spec.data_ptr(), None, 2 * n, rows)}
    with torch.cuda.stream(stream):
        times = abtime.alternate(stream, calls, warmup=3, rounds=5, reps=10)
    frac = lambda ms: 8 * n * rows / (ms * 1e-3) / 8e12
    line = f"n {n:6d} rows {rows:9d}:"
    for k, t in times.items():
        md = float(np.median(t))
        line += f" | {k} {abtime.cell(t)}" + (f" {frac(md):.3f}" if k != "rfft" else "")
    print(line, flush=True)
    del x, y, mirrored, spec
    torch.cuda.empty_cache()
