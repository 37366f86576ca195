"""hilbert::hilbert_analytic (hilbert.rs:13-47) on device memory over row lengths: 2^28 input floats per call (1 GiB of rows in, 2 GiB
of complex64 out), HIP events.  In one process a default context (fused kernel for powers of two 32 .. 4096) alternates with a
set_hilbert_fused(False) context (expand kernel -> n-point transform -> mask kernel -> inverse transform) and with what a caller ran on
the device without this entry point: widen to complex in torch, fft_dev, a torch mask, inverse fft_dev.  Five rounds of 10 timed
calls each, after 3 warm-up calls; median [min .. max] ms per call.  Fraction of the roofline: 8 TB/s on 12 bytes per point (4 in,
8 out).
usage: bench_hilbert.py [n ...]"""
import sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime
fused = kofft_amd.HipFftImpl(np.float32)
composed = kofft_amd.HipFftImpl(np.float32)
composed.set_hilbert_fused(False)
stream = abtime.one_stream(fused, composed)


def by_hand(x, y, n, rows):
    """What a caller ran before: (x, 0), forward transform in place, mask in torch, inverse transform in place."""
    yr = torch.view_as_real(y)
    yr[..., 0].copy_(x)
    yr[..., 1].zero_()
    fused.fft_dev(y.data_ptr(), n, rows, False)
    if n > 2:
        yr[:, 1:n // 2].mul_(2.0)
        y[:, n // 2 + 1:].zero_()
    fused.fft_dev(y.data_ptr(), n, rows, True)


for n in [int(a) for a in sys.argv[1:]] or [8, 64, 256, 1024, 4096, 16384, 65536]:
    rows = (1 << 28) // n
    x = torch.empty((rows, n), dtype=torch.float32, device="cuda").uniform_(-1, 1)
    y = torch.empty((rows, n), dtype=torch.complex64, device="cuda")
    calls = {"fused": lambda: fused.hilbert_dev(x.data_ptr(), y.data_ptr(), n, rows),
             "composed": lambda: composed.hilbert_dev(x.data_ptr(), y.data_ptr(), n, rows),
             "by hand": lambda: by_hand(x, y, n, rows)}
    with torch.cuda.stream(stream):
        times = abtime.alternate(stream, calls, warmup=3, rounds=5, reps=10)
    frac = lambda ms: 12 * n * rows / (ms * 1e-3) / 8e12
    line = f"n {n:6d} rows {rows:9d}:"
    for k, t in times.items():
        md = float(np.median(t))
        line += f" | {k} {abtime.cell(t)} {frac(md):.3f}"
    print(line, flush=True)
    del x, y
    torch.cuda.empty_cache()
