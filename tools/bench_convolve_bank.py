"""Filter-bank overlap-save convolution of rows on device memory, "full" windows, HIP events.  In one process a default
context (the fused bank kernel for blocks 32 .. 4096) alternates with a set_convolve_bank_fused(False) context (frames into the scratch
and transformed once, then per filter multiply -> inverse transform -> gather) and with what a caller ran without this entry point:
`filters` calls of convolve_dev, one filter each, on the same signal into one row-sized buffer (complex taps: two calls per filter, the
real and the imaginary taps, and no combining pass -- less than such a caller needs).  Five rounds of 10 timed calls each, after 3
warm-up calls; median [min .. max] ms per call.  Fraction of the roofline: 8 TB/s on 4 nx + elem filters out_len bytes per row (elem 4,
or 8 for complex values).  The tool is one GPU step per invocation: run each shape under its own `timeout`.
usage: bench_convolve_bank.py [rows nx nh block filters taps kind ...]   (groups of seven; taps: real | complex; kind: real | complex |
       magnitude; none: the shapes of DESIGN.md 5.31)"""
import sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime
fused = kofft_amd.HipFftImpl(np.float32)
composed = kofft_amd.HipFftImpl(np.float32)
composed.set_convolve_bank_fused(False)
stream = abtime.one_stream(fused, composed)


def one_by_one(x, h, one, rows, nx, nh, block, calls):
    """What a caller ran before: one convolve_dev per filter (calls: filters, or 2 filters for complex taps) on the same signal."""
    for f in range(calls):
        fused.convolve_dev(x.data_ptr(), rows, nx, h.data_ptr() + 4 * nh * f, 1, nh, one.data_ptr(), block)


# The 4096 x 16000 shape with 40 filters would write 10.7 GB (21 GB of complex values): it runs on 2048 rows (1024 for complex values),
# 5.4 GB, so that every output stays below 8 GB.
DEFAULT = ([(16, 1 << 21, 512, 2048, fl, "real", k) for fl in (4, 32) for k in ("real", "magnitude")]
           + [(16, 1 << 21, 2001, 4096, 32, "real", k) for k in ("real", "magnitude")]
           + [(2048, 16000, 401, 1024, 40, "real", k) for k in ("real", "magnitude")]
           + [(2048, 16000, 401, 1024, 40, "complex", "magnitude"), (1024, 16000, 401, 1024, 40, "complex", "complex")])
args = sys.argv[1:]
shapes = [tuple(int(a) for a in args[i:i + 5]) + tuple(args[i + 5:i + 7]) for i in range(0, len(args), 7)] or DEFAULT
last = None
for rows, nx, nh, block, filters, taps, kind in shapes:
    full = nx + nh - 1
    cplx, elem = taps == "complex", 8 if kind == "complex" else 4
    assert rows * filters * full * elem <= 8e9, "an output above 8 GB"
    if last != (rows, nx):
        x = torch.empty((rows, nx), dtype=torch.float32, device="cuda").uniform_(-1, 1)
        last = (rows, nx)
    h = torch.empty(filters * nh * (2 if cplx else 1), dtype=torch.float32, device="cuda").uniform_(-1, 1)
    out = torch.empty(rows * filters * full * elem // 4, dtype=torch.float32, device="cuda")
    one = torch.empty((rows, full), dtype=torch.float32, device="cuda")
    bank = lambda f: f.convolve_bank_dev(x.data_ptr(), rows, nx, h.data_ptr(), filters, nh, out.data_ptr(), block, complex_taps=cplx,
                                         out=kind)
    calls = {"fused": lambda: bank(fused), "composed": lambda: bank(composed),
             "one by one": lambda: one_by_one(x, h, one, rows, nx, nh, block, filters * (2 if cplx else 1))}
    with torch.cuda.stream(stream):
        times = abtime.alternate(stream, calls, warmup=3, rounds=5, reps=10)
    frac = lambda ms: (4.0 * nx + elem * filters * full) * rows / (ms * 1e-3) / 8e12
    line = f"rows {rows:5d} nx {nx:8d} nh {nh:5d} block {block:5d} filters {filters:3d} taps {taps:7s} out {kind:9s}:"
    for k, t in times.items():
        md = float(np.median(t))
        line += f" | {k} {abtime.cell(t)} {frac(md):.3f}"
    md = {k: float(np.median(t)) for k, t in times.items()}
    line += f" | one by one / fused {md['one by one'] / md['fused']:.2f} (bound {2 * filters / (filters + 1):.2f})"
    print(line, flush=True)
    del h, out, one
    torch.cuda.empty_cache()
