"""cepstrum::real_cepstrum (cepstrum.rs:12-33) on device memory over row lengths: 2^28 input floats per call (1 GiB of rows in, 1 GiB
out), HIP events.  In one process a default context (fused kernel for powers of two 32 .. 4096) alternates with a
set_cepstrum_fused(False) context (expand kernel -> n-point transform -> log-magnitude kernel -> inverse transform -> real parts, through
the context's scratch) and with what a caller ran on the device without this entry point: widen to complex in torch, fft_dev, the
log-magnitude in torch, inverse fft_dev, the real parts in torch.  Five rounds of 10 timed calls each, after 3 warm-up calls;
median [min .. max] ms per call.  Fraction of the roofline: 8 TB/s on 8 bytes per point (4 in, 4 out).
usage: bench_cepstrum.py [n ...]"""
import sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime
fused = kofft_amd.HipFftImpl(np.float32)
composed = kofft_amd.HipFftImpl(np.float32)
composed.set_cepstrum_fused(False)
stream = abtime.one_stream(fused, composed)


def by_hand(x, y, out, n, rows):
    """What a caller ran before: (x, 0), forward transform in place, log-magnitude in torch, inverse transform in place, real parts."""
    yr = torch.view_as_real(y)
    yr[..., 0].copy_(x)
    yr[..., 1].zero_()
    if n > 1:
        fused.fft_dev(y.data_ptr(), n, rows, False)
    yr[..., 0].copy_(torch.log(torch.abs(y) + 1e-12))
    yr[..., 1].zero_()
    if n > 1:
        fused.fft_dev(y.data_ptr(), n, rows, True)
    out.copy_(yr[..., 0])


for n in [int(a) for a in sys.argv[1:]] or [8, 64, 256, 1024, 4096, 16384, 65536]:
    rows = (1 << 28) // n
    x = torch.empty((rows, n), dtype=torch.float32, device="cuda").uniform_(-1, 1)
    out = torch.empty((rows, n), dtype=torch.float32, device="cuda")
    y = torch.empty((rows, n), dtype=torch.complex64, device="cuda")
    calls = {"fused": lambda: fused.cepstrum_dev(x.data_ptr(), out.data_ptr(), n, rows),
             "composed": lambda: composed.cepstrum_dev(x.data_ptr(), out.data_ptr(), n, rows),
             "by hand": lambda: by_hand(x, y, out, n, rows)}
    with torch.cuda.stream(stream):
        times = abtime.alternate(stream, calls, warmup=3, rounds=5, reps=10)
    frac = lambda ms: 8 * n * rows / (ms * 1e-3) / 8e12
    line = f"n {n:6d} rows {rows:9d}:"
    for k, t in times.items():
        md = float(np.median(t))
        line += f" | {k} {abtime.cell(t)} {frac(md):.3f}"
    print(line, flush=True)
    del x, out, y
    torch.cuda.empty_cache()
