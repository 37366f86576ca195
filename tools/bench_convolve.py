"""Overlap-save convolution of rows on device memory, "full" windows, HIP events.  In one process a default context
(fused kernel for blocks 32 .. 4096) alternates with a set_convolve_fused(False) context (frames into the scratch -> transform ->
multiply -> inverse transform -> gather) and with what a caller ran on the device without this entry point: widen each row to
next_pow2(nx + nh - 1) complex points in torch, fft_dev, a torch multiply by the filter's spectrum, inverse fft_dev, slice.  Five rounds
of 10 timed calls each, after 3 warm-up calls; median [min .. max] ms per call.  Fraction of the roofline: 8 TB/s on 4 nx + 4 out_len
bytes per row.
usage: bench_convolve.py [rows nx nh block ...]      (groups of four; none: the shapes of DESIGN.md 5.25)"""
import sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime
fused = kofft_amd.HipFftImpl(np.float32)
composed = kofft_amd.HipFftImpl(np.float32)
composed.set_convolve_fused(False)
stream = abtime.one_stream(fused, composed)


def by_hand(x, h, z, hz, out, n, rows, nx, nh):
    """What a caller ran before: (x, 0) zero-padded to n points, forward transform, the product in torch, inverse transform, slice."""
    z.zero_()
    torch.view_as_real(z)[:, :nx, 0].copy_(x)
    hz.zero_()
    torch.view_as_real(hz)[:nh, 0].copy_(h)
    fused.fft_dev(hz.data_ptr(), n, 1, False)
    fused.fft_dev(z.data_ptr(), n, rows, False)
    z.mul_(hz)
    fused.fft_dev(z.data_ptr(), n, rows, True)
    out.copy_(torch.view_as_real(z)[:, :nx + nh - 1, 0])


args = [int(a) for a in sys.argv[1:]]
shapes = [tuple(args[i:i + 4]) for i in range(0, len(args), 4)] or (
    [(16, 1 << 24, nh, b) for nh in (64, 512, 2048) for b in (1024, 2048, 4096) if b >= 2 * nh]
    + [(65536, 3000, 1097, 4096), (1 << 20, 200, 57, 256)])
last = None
for rows, nx, nh, block in shapes:
    full = nx + nh - 1
    n = 1 << (full - 1).bit_length()
    if last != (rows, nx):
        x = torch.empty((rows, nx), dtype=torch.float32, device="cuda").uniform_(-1, 1)
        last = (rows, nx)
    h = torch.empty(nh, dtype=torch.float32, device="cuda").uniform_(-1, 1)
    out = torch.empty((rows, full), dtype=torch.float32, device="cuda")
    z = torch.empty((rows, n), dtype=torch.complex64, device="cuda")
    hz = torch.empty(n, dtype=torch.complex64, device="cuda")
    calls = {"fused": lambda: fused.convolve_dev(x.data_ptr(), rows, nx, h.data_ptr(), 1, nh, out.data_ptr(), block),
             "composed": lambda: composed.convolve_dev(x.data_ptr(), rows, nx, h.data_ptr(), 1, nh, out.data_ptr(), block),
             "by hand": lambda: by_hand(x, h, z, hz, out, n, rows, nx, nh)}
    with torch.cuda.stream(stream):
        times = abtime.alternate(stream, calls, warmup=3, rounds=5, reps=10)
    frac = lambda ms: 4.0 * (nx + full) * rows / (ms * 1e-3) / 8e12
    line = f"rows {rows:8d} nx {nx:9d} nh {nh:5d} block {block:5d}:"
    for k, t in times.items():
        line += f" | {k} {abtime.cell(t)} {frac(float(np.median(t))):.3f}"
    print(line, flush=True)
    del h, out, z, hz
    torch.cuda.empty_cache()
