"""The polyphase filter bank of rows, analysis and synthesis, on device memory, HIP events.  In one process on one
stream a set_pfb_fused(2) context (pfb_fused_kernel / pfb_inverse_fused_kernel for M = 32 .. 4096) alternates with a set_pfb_fused(False)
context (fold kernel -> M-point transform -> prefix copy; completion -> inverse transform -> real parts), and, for the sweep, with
the fast DCT-IV of rows of the same length (dct4_fused_kernel, the toolkit's neighbour) on the same number of items.  Five rounds of timed calls
after 3 warm-up calls; median [min .. max] ms per call, and the fraction of the roofline: 8 TB/s over the bytes the definition must
move (the samples in once, the bins out once; the synthesis the other way round).
  shapes: 1: 16 x 2^21 samples, M = 1024, T = 4, D = 1024, one-sided;  2: 2048 x 16000 samples, M = 256, T = 8, D = 128, one-sided;
          3: 16 x 2^21 samples, M = 4096, T = 16, D = 4096, one-sided;  each followed by its synthesis
  sweep:  2^25 samples in 16 rows, M = 32 .. 8192, T = 4, D = M, all M bins
usage: bench_pfb.py [shapes [1 2 3]] [sweep [M ...]]      (no argument: everything)"""
import sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime
from kofft_amd import pfb

fused = kofft_amd.HipFftImpl(np.float32)
fused.set_pfb_fused(2)  # the fused kernels wherever they exist: the default context takes the faster of the two columns
composed = kofft_amd.HipFftImpl(np.float32)
composed.set_pfb_fused(False)
stream = abtime.one_stream(fused, composed)
SHAPES = {1: (16, 1 << 21, 1024, 4, 1024), 2: (2048, 16000, 256, 8, 128), 3: (16, 1 << 21, 4096, 16, 4096)}


def report(head, times, nbytes):
    line = head
    for k, t in times.items():
        md = float(np.median(t))
        line += f" | {k} {abtime.cell(t)} {nbytes / (md * 1e-3) / 8e12:.3f}"
    print(line, flush=True)


def bench(head, rows, nx, m, taps, hop, bins, with_dct4=False):
    nh = taps * m
    lead = nh - hop
    frames = -(-(nx + lead) // hop)
    x = torch.empty((rows, nx), dtype=torch.float32, device="cuda").uniform_(-1, 1)
    h = torch.from_numpy(pfb.prototype(m, taps)).cuda()
    Z = torch.empty((rows, frames, bins, 2), dtype=torch.float32, device="cuda")
    back = torch.empty_like(x)
    torch.cuda.synchronize()
    ctxs = {"fused" if 32 <= m <= 4096 else "default": fused, "composed": composed}
    head = f"{head} ({rows} x {nx}, M {m}, T {taps}, D {hop}, {frames} frames, {bins} bins)"
    nbytes = 4 * rows * nx + 8 * Z.numel() // 2
    with torch.cuda.stream(stream):
        fwd = {k: (lambda f=f: f.pfb_analysis_dev(x.data_ptr(), rows, nx, nx, h.data_ptr(), nh, m, hop, lead, Z.data_ptr(), frames, bins))
               for k, f in ctxs.items()}
        if with_dct4 and 64 <= m <= 8192:  # the same number of items of the same length through the neighbouring fused kernel
            u = torch.empty((rows * frames, m), dtype=torch.float32, device="cuda").uniform_(-1, 1)
            v = torch.empty_like(u)
            fwd["dct4"] = lambda: fused.dct4_fast_dev(u.data_ptr(), v.data_ptr(), m, rows * frames)
        report(head + " analysis: ", abtime.alternate(stream, fwd, warmup=3, rounds=5, reps=10), nbytes)
        inv = {k: (lambda f=f: f.pfb_synthesis_dev(Z.data_ptr(), rows, frames, bins, h.data_ptr(), nh, m, hop, 1.0, back.data_ptr(), lead, nx))
               for k, f in ctxs.items()}
        report(head + " synthesis:", abtime.alternate(stream, inv, warmup=3, rounds=5, reps=10), nbytes)


args = sys.argv[1:]
mode, picked = None, {"shapes": [], "sweep": []}
for a in args:
    if a in picked:
        mode = a
    else:
        picked[mode].append(int(a))
run_all = not args
if run_all or "shapes" in args:
    for which in picked["shapes"] or [1, 2, 3]:
        rows, nx, m, taps, hop = SHAPES[which]
        bench(f"shape {which}", rows, nx, m, taps, hop, m // 2 + 1)
        torch.cuda.empty_cache()
if run_all or "sweep" in args:
    for m in picked["sweep"] or [32 << i for i in range(9)]:
        bench("sweep", 16, 1 << 21, m, 4, m, m, with_dct4=True)
        torch.cuda.empty_cache()
