"""Polyphase resampling of rows on device memory, resample_poly's window (t0 = (nh - 1) // 2, ceil(nx up / down)
outputs), HIP events.  In one process a set_resample_tiled(2) context (the tiled kernel wherever its tables fit), a
set_resample_tiled(0) context (the plain kernel) and the default context alternate with what a caller ran on the device without this
entry point: zero-stuff the rows by `up` in torch, kofft_amd.convolve on the device at its default block, keep every `down`-th value
(only where rows * nx * up floats fit 2^31; with up == down == 1 that column is the FFT convolution itself).  Five rounds of 10 timed
calls each, after 3 warm-up calls; median [min .. max] ms per call.  Fraction of the roofline: 8 TB/s on 4 nx + 4 out_len bytes per row.
usage: bench_resample.py [rows nx up down nh ...]      (groups of five, nh 0: design_taps(up, down); none: the shapes of DESIGN.md 5.28)"""
import sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime
from kofft_amd import resample
ctxs = {"tiled": kofft_amd.HipFftImpl(np.float32), "plain": kofft_amd.HipFftImpl(np.float32), "default": kofft_amd.HipFftImpl(np.float32)}
ctxs["tiled"].set_resample_tiled(2)
ctxs["plain"].set_resample_tiled(0)
stream = abtime.one_stream(*ctxs.values())
conv = ctxs["default"]


def by_hand(x, h, xu, full, out, rows, nx, nh, up, down, t0, out_len):
    """What a caller ran before: the rows zero-stuffed by up, the FFT convolution's full result, every down-th value from t0."""
    src = x
    if up > 1:
        xu.zero_()
        xu[:, ::up].copy_(x)
        src = xu
    conv.convolve_dev(src.data_ptr(), rows, nx * up, h.data_ptr(), 1, nh, full.data_ptr())
    out.copy_(full[:, t0::down][:, :out_len])


args = [int(a) for a in sys.argv[1:]]
shapes = [tuple(args[i:i + 5]) for i in range(0, len(args), 5)] or [
    (16, 1 << 24, 1, 3, 0), (16, 1 << 24, 160, 441, 0), (16, 1 << 24, 3, 1, 0), (65536, 3000, 1, 3, 0), (1 << 20, 200, 2, 1, 0),
    (16, 1 << 24, 1, 1, 64)]
last = None
for rows, nx, up, down, nh in shapes:
    if nh == 0:
        h = torch.from_numpy(resample.design_taps(up, down)).cuda()
    else:
        h = torch.empty(nh, dtype=torch.float32, device="cuda").uniform_(-1, 1)
    nh = h.numel()
    t0 = (nh - 1) // 2
    out_len = min(-(-nx * up // down), -(-((nx - 1) * up + nh - t0) // down))
    if last != (rows, nx):
        x = torch.empty((rows, nx), dtype=torch.float32, device="cuda").uniform_(-1, 1)
        last = (rows, nx)
    out = torch.empty((rows, out_len), dtype=torch.float32, device="cuda")
    route = resample.route(nh, up, down)
    calls = {k: (lambda f=f: f.resample_dev(x.data_ptr(), rows, nx, h.data_ptr(), nh, up, down, t0, out.data_ptr(), out_len))
             for k, f in ctxs.items()}
    xu = full = None
    if rows * nx * up < (1 << 31):
        xu = torch.empty((rows, nx * up), dtype=torch.float32, device="cuda") if up > 1 else None
        full = torch.empty((rows, nx * up + nh - 1), dtype=torch.float32, device="cuda")
        calls["by hand"] = lambda: by_hand(x, h, xu, full, out, rows, nx, nh, up, down, t0, out_len)
    with torch.cuda.stream(stream):
        times = abtime.alternate(stream, calls, warmup=3, rounds=5, reps=10)
    frac = lambda ms: 4.0 * (nx + out_len) * rows / (ms * 1e-3) / 8e12
    line = f"rows {rows:8d} nx {nx:9d} {up:3d}/{down:3d} nh {nh:5d} out {out_len:9d} route {route}:"
    for k, t in times.items():
        md = float(np.median(t))
        line += f" | {k} {abtime.cell(t)} {frac(md):.3f}"
    print(line, flush=True)
    del h, out, xu, full
    torch.cuda.empty_cache()
