"""FftImpl::fft_split / ifft_split (fft.rs:1365-1439) on device-resident planes over row lengths: 2^27 points per call (f32: 512 MiB of
planes in, 512 MiB out; f64 twice that), HIP events.  In one process a default context (PlanarIO in the one-workgroup kernels: one launch on
the planes) alternates with a set_split_fused(False) context (pack kernel -> n-point transform in the context's scratch -> unpack kernel) and,
as a yardstick, with fft_dev on interleaved data of the same shape.  Five rounds of 10 timed calls each, after 3 warm-up calls; median
[min .. max] ms per call.  Fraction of the roofline: 8 TB/s on 16 bytes per point (f64: 32), what the transform itself has to move.
usage: bench_split.py [f32|f64|both] [n ...]"""
import sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime
args = sys.argv[1:]
which = args.pop(0) if args and args[0] in ("f32", "f64", "both") else "both"
sizes = [int(a) for a in args] or [8, 64, 256, 1024, 4096, 16384]
stream = abtime.one_stream()
POINTS = 1 << 27


for real, tdt, cdt in [(np.float32, torch.float32, torch.complex64), (np.float64, torch.float64, torch.complex128)]:
    if which not in ("both", np.dtype(real).name.replace("float", "f")):
        continue
    fused = kofft_amd.HipFftImpl(real)
    composed = kofft_amd.HipFftImpl(real)
    composed.set_split_fused(False)
    for f in (fused, composed):
        f.set_stream(stream.cuda_stream)
    item = np.dtype(real).itemsize
    for n in sizes:
        if n > (1 << (14 if real == np.float32 else 13)):
            continue  # (the fused route ends there)
        rows = POINTS // n
        re = torch.empty((rows, n), dtype=tdt, device="cuda").uniform_(-1, 1)
        im = torch.empty((rows, n), dtype=tdt, device="cuda").uniform_(-1, 1)
        o_re, o_im = torch.empty_like(re), torch.empty_like(im)
        z = torch.empty((rows, n), dtype=cdt, device="cuda")
        torch.view_as_real(z).uniform_(-1, 1)
        zo = torch.empty_like(z)
        calls = {"fused": lambda: fused.fft_split_dev(re, im, o_re, o_im),
                 "composed": lambda: composed.fft_split_dev(re, im, o_re, o_im),
                 "interleaved": lambda: fused.fft_dev_oop(z.data_ptr(), zo.data_ptr(), n, rows)}
        with torch.cuda.stream(stream):
            times = abtime.alternate(stream, calls, warmup=3, rounds=5, reps=10)
        frac = lambda ms: 4 * item * n * rows / (ms * 1e-3) / 8e12
        line = f"{np.dtype(real).name} n {n:6d} rows {rows:9d}:"
        for k, t in times.items():
            md = float(np.median(t))
            line += f" | {k} {abtime.cell(t)} {frac(md):.3f}"
        print(line, flush=True)
        del re, im, o_re, o_im, z, zo
        torch.cuda.empty_cache()
    for f in (fused, composed):
        f.set_stream(0)
        f.close()
