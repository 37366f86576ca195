"""Rows of audio to MFCCs on device memory (kofft_hip_dev_stft_mfcc_f32), HIP events, one process.  Routes, alternating: the CHAIN --
the two calls a caller made before this entry existed, stft_magnitudes_rows_dev into a caller-owned magnitudes buffer, then mfcc_dev:
the yardstick --, the FUSED kernel (set_frontend_fused(2)), the COMPOSED route (set_frontend_fused(0): magnitudes without a maximum into
the context's scratch, then the MFCC path) and the DEFAULT (mode 1).  Before timing, every route's result is compared with the
chain's bit for bit at the timed size.  Five rounds of 10 timed calls each, after 3 warm-up calls; median [min .. max] ms per call.
Shapes (rows, len, win_len, hop, filters, coefficients): config 4's stream, 4096 clips of one second at 512 / 160, 64 clips of ten
seconds at 2048 / 512, and one shape per fused window length at 40 x 13 in two batch sizes.
usage: bench_frontend.py [shape index | rows,len,win_len,hop,filters,coefficients ...]"""
import sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime
from kofft_amd import mfcc
SHAPES = [(1, 28_800_000, 1024, 256, 40, 13), (4096, 16000, 512, 160, 26, 13), (64, 480_000, 2048, 512, 80, 13)]
SHAPES += [(rows, (1 << 24) // 64 * 64 // rows, w, w // 4, 40, 13) for w in (64, 128, 256, 512, 1024, 2048) for rows in (64, 1024)]
ctx = {}
for name, mode in (("chain", 1), ("fused", 2), ("composed", 0), ("default", 1)):
    ctx[name] = kofft_amd.HipFftImpl(np.float32)
    ctx[name].set_frontend_fused(mode)
stream = abtime.one_stream(*ctx.values())


for arg in sys.argv[1:] or range(len(SHAPES)):
    rows, length, win_len, hop, num_mel, nc = [int(v) for v in arg.split(",")] if "," in str(arg) else SHAPES[int(arg)]
    frames, n_fft = -(-length // hop), win_len // 2
    bins = mfcc.mel_bins(16000.0, n_fft, num_mel)
    x = torch.empty((rows, length), dtype=torch.float32, device="cuda").normal_()
    mags = torch.empty((rows * frames, n_fft), dtype=torch.float32, device="cuda")
    mx = torch.empty((rows,), dtype=torch.float32, device="cuda")
    out = {k: torch.empty((rows * frames, nc), dtype=torch.float32, device="cuda") for k in ctx}

    def chain():
        f = ctx["chain"]
        f.stft_magnitudes_rows_dev(x.data_ptr(), rows, length, length, win_len, hop, mags.data_ptr(), frames, mx.data_ptr())
        f.mfcc_dev(mags.data_ptr(), out["chain"].data_ptr(), n_fft, rows * frames, bins, nc)

    def one(k):
        return lambda: ctx[k].stft_mfcc_rows_dev(x.data_ptr(), rows, length, length, 0, win_len, hop, frames, bins, nc, out[k].data_ptr())

    calls = {"chain": chain, "fused": one("fused"), "composed": one("composed"), "default": one("default")}
    times = {k: [] for k in calls}
    with torch.cuda.stream(stream):
        for c in calls.values():
            for _ in range(3):
                c()
        torch.cuda.synchronize()
        same = {k: torch.equal(out[k].view(torch.int32), out["chain"].view(torch.int32)) for k in calls if k != "chain"}
        for _ in range(5):
            for k, c in calls.items():
                times[k].append(abtime.timed(stream, c))
    line = f"rows {rows:5d} len {length:9d} win {win_len:5d} hop {hop:4d} mel {num_mel:3d} coeffs {nc:3d} frames {rows * frames:8d} == chain: {same}:"
    for k, t in times.items():
        line += f" | {k} {abtime.cell(t)}"
    print(line, flush=True)
    del x, mags, mx, out
    torch.cuda.empty_cache()
