"""cepstrum::mfcc (cepstrum.rs:72-85) on device memory at three shapes (rows x n_fft, filters, coefficients): config 4's spectrogram
(112500 x 512, 40, 13), 2^20 x 256 (26, 13) and 4096 x 1024 (128, 128), reference-shaped edges at 16 kHz, HIP events.  In one process a
set_mfcc_fused(2) context (the fused kernel) alternates with a set_mfcc_fused(0) context (filterbank kernel -> log kernel -> direct DCT-II ->
column copy, through the context's scratch), with the filterbank alone, and with a dense torch pipeline (filter matrix matmul, log, DCT
matmul): a timing yardstick only, it does not produce the reference's bytes.  Before timing, the fused and the composed results are
compared bit for bit at the timed size.  Five rounds of 10 timed calls each, after 3 warm-up calls; median [min .. max] ms per call.
Fraction of the roofline: 8 TB/s on rows * (n_fft + num_coeffs) * 4 bytes.
usage: bench_mfcc.py [shape index | rows,n_fft,filters,coefficients ...]"""
import sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime
from kofft_amd import mfcc
SHAPES = [(112500, 512, 40, 13), (1 << 20, 256, 26, 13), (4096, 1024, 128, 128)]
fused = kofft_amd.HipFftImpl(np.float32)
fused.set_mfcc_fused(2)  # the fused kernel wherever it fits, also where the default takes the composed route
composed = kofft_amd.HipFftImpl(np.float32)
composed.set_mfcc_fused(0)
stream = abtime.one_stream(fused, composed)


def dense(bins, n_fft, num_mel, nc):
    """The filter matrix [n_fft, num_mel] and the DCT-II matrix [num_mel, nc] of the dense pipeline."""
    w = np.zeros((n_fft, num_mel), np.float32)
    for m in range(num_mel):
        a, b, c = (int(v) for v in bins[m:m + 3])
        if b == a or c == b:
            continue
        for k in range(a, min(b, n_fft)):
            w[k, m] = (k - a) / (b - a)
        for k in range(b, min(c, n_fft)):
            w[k, m] = (c - k) / (c - b)
    i, j = np.arange(num_mel)[:, None], np.arange(nc)[None, :]
    d = np.cos(np.pi / num_mel * (i + 0.5) * j).astype(np.float32)
    return torch.from_numpy(w).cuda(), torch.from_numpy(d).cuda()


for arg in sys.argv[1:] or range(len(SHAPES)):
    rows, n_fft, num_mel, nc = [int(v) for v in arg.split(",")] if "," in str(arg) else SHAPES[int(arg)]
    bins = mfcc.mel_bins(16000.0, n_fft, num_mel)
    x = torch.empty((rows, n_fft), dtype=torch.float32, device="cuda").uniform_(0, 1)
    out = torch.empty((rows, nc), dtype=torch.float32, device="cuda")
    out2 = torch.empty((rows, nc), dtype=torch.float32, device="cuda")
    en = torch.empty((rows, num_mel), dtype=torch.float32, device="cuda")
    w, d = dense(bins, n_fft, num_mel, nc)
    calls = {"fused": lambda: fused.mfcc_dev(x.data_ptr(), out.data_ptr(), n_fft, rows, bins, nc),
             "composed": lambda: composed.mfcc_dev(x.data_ptr(), out2.data_ptr(), n_fft, rows, bins, nc),
             "filterbank": lambda: fused.mel_filterbank_dev(x.data_ptr(), en.data_ptr(), n_fft, rows, bins),
             "torch dense": lambda: torch.matmul(torch.log(torch.matmul(x, w) + 1e-12), d)}
    times = {k: [] for k in calls}
    with torch.cuda.stream(stream):
        for c in calls.values():
            for _ in range(3):
                c()
        torch.cuda.synchronize()
        same = torch.equal(out.view(torch.int32), out2.view(torch.int32))
        for _ in range(5):
            for k, c in calls.items():
                times[k].append(abtime.timed(stream, c))
    frac = lambda ms: 4 * rows * (n_fft + nc) / (ms * 1e-3) / 8e12
    line = f"rows {rows:8d} n_fft {n_fft:5d} mel {num_mel:4d} coeffs {nc:4d} fused == composed: {same}:"
    for k, t in times.items():
        md = float(np.median(t))
        line += f" | {k} {abtime.cell(t)} {frac(md):.3f}"
    print(line, flush=True)
    del x, out, out2, en, w, d
    torch.cuda.empty_cache()
