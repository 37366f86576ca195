"""The fast DCT-IV, MDCT and IMDCT of rows on device memory, HIP events.  In one process on one stream a default
context (dct4_fused_kernel for N = 64 .. 8192) alternates with a set_mdct_fused(False) context (fold / pre-twiddle kernel -> N/2-point
transform -> post-twiddle kernel) and, for the DCT-IV rows up to N = 4096, with the reference's direct sum dct::dct4 (dct_direct_dev).
Five rounds of timed calls after 3 warm-up calls; median [min .. max] ms per call, and the fraction of the roofline: 8 TB/s over the
bytes the definition must move (the samples or coefficients in once, the results out once).
  dct4:   2^28 input floats per call at N = 64, 256, 1024, 4096, 8192, 16384, 65536
  shapes: 1: 16 x 2^21 samples, N = 1024;  2: 2048 x 16000 samples, N = 256;  3: 16 x 2^21 samples, N = 960 (composed only)
usage: bench_mdct.py [dct4 [N ...]] [shapes [1 2 3]]      (no argument: everything)"""
import sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime
from kofft_amd import mdct as km

fused = kofft_amd.HipFftImpl(np.float32)
composed = kofft_amd.HipFftImpl(np.float32)
composed.set_mdct_fused(False)
stream = abtime.one_stream(fused, composed)
SHAPES = {1: (16, 1 << 21, 1024), 2: (2048, 16000, 256), 3: (16, 1 << 21, 960)}


def report(head, times, nbytes):
    line = head
    for k, t in times.items():
        md = float(np.median(t))
        line += f" | {k} {abtime.cell(t)} {nbytes / (md * 1e-3) / 8e12:.3f}"
    print(line, flush=True)


def bench_dct4(n):
    rows = (1 << 28) // n
    x = torch.empty((rows, n), dtype=torch.float32, device="cuda").uniform_(-1, 1)
    y = torch.empty_like(x)
    calls = {"fused" if 64 <= n <= 8192 and n & (n - 1) == 0 else "default": lambda: fused.dct4_fast_dev(x.data_ptr(), y.data_ptr(), n, rows),
             "composed": lambda: composed.dct4_fast_dev(x.data_ptr(), y.data_ptr(), n, rows)}
    reps = {k: 10 for k in calls}
    if n <= 4096:
        calls["direct"] = lambda: fused.dct_direct_dev(4, x.data_ptr(), y.data_ptr(), n, rows)
        reps["direct"] = 10 if n <= 256 else 2
    with torch.cuda.stream(stream):
        times = abtime.alternate(stream, calls, warmup=3, rounds=5, reps=reps)
    report(f"dct4 N {n:6d} rows {rows:8d}:", times, 8 * n * rows)


def bench_shape(which):
    rows, nx, n = SHAPES[which]
    frames = -(-nx // n) + 1
    x = torch.empty((rows, nx), dtype=torch.float32, device="cuda").uniform_(-1, 1)
    w = torch.from_numpy(km.sine_window(n)).cuda()
    X = torch.empty((rows, frames, n), dtype=torch.float32, device="cuda")
    back = torch.empty_like(x)
    torch.cuda.synchronize()
    ctxs = {"composed": composed} if which == 3 else {"fused": fused, "composed": composed}
    head = f"shape {which} ({rows} x {nx}, N {n}, {frames} frames)"
    with torch.cuda.stream(stream):
        fwd = {k: (lambda f=f: f.mdct_dev(x.data_ptr(), rows, nx, nx, w.data_ptr(), n, n, X.data_ptr(), frames)) for k, f in ctxs.items()}
        times = abtime.alternate(stream, fwd, warmup=3, rounds=5, reps=10)
        report(head + " mdct: ", times, 4 * (rows * nx + X.numel()))
        inv = {k: (lambda f=f: f.imdct_dev(X.data_ptr(), rows, frames, w.data_ptr(), n, 2.0 / n, back.data_ptr(), n, nx)) for k, f in ctxs.items()}
        times = abtime.alternate(stream, inv, warmup=3, rounds=5, reps=10)
        report(head + " imdct:", times, 4 * (rows * nx + X.numel()))
    err = float(torch.linalg.norm(back - x) / torch.linalg.norm(x))
    print(f"{head} round trip: relative L2 error {err:.3g}", flush=True)


args = sys.argv[1:]
mode, picked = None, {"dct4": [], "shapes": []}
for a in args:
    if a in picked:
        mode = a
    else:
        picked[mode].append(int(a))
run_all = not args
if run_all or "dct4" in args:
    for n in picked["dct4"] or [64, 256, 1024, 4096, 8192, 16384, 65536]:
        bench_dct4(n)
        torch.cuda.empty_cache()
if run_all or "shapes" in args:
    for which in picked["shapes"] or [1, 2, 3]:
        bench_shape(which)
        torch.cuda.empty_cache()
