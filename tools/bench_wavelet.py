"""The wavelet transforms on device memory, HIP events, all five wavelets.
Single level: dwt / idwt (the streaming kernels) over row lengths.  Multi level: three contexts alternate in one process -- the
fused kernels wherever the row fits (set_wavelet_fused(2)), level by level on the streaming kernels (set_wavelet_fused(False)) and
the default, which picks between them by the table these numbers fill (k_wavelet_f32.hip: kFusedAuto) -- at levels 1, 2, 3, 5 and 8,
forward (wavedec_dev) and inverse (waverec_dev).  Every call moves 64 M input floats; each timed sample runs enough calls for
>= ~5 ms.  Five rounds after 3 warm-up calls; median [min .. max] ms per call.  Reported: the share of 8 TB/s counting 8 bytes per
input point (one read, one write), and the fused and default routes against the per-level one.
usage: bench_wavelet.py [n ...]"""
import sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime

stream = abtime.one_stream()
NAMES = ("haar", "db2", "db4", "sym4", "coif1")


def ctx(mode):
    f = kofft_amd.HipFftImpl(np.float32)
    f.set_wavelet_fused(mode)
    f.set_stream(stream.cuda_stream)
    return f


def measure(calls):
    with torch.cuda.stream(stream):
        for c in calls.values():
            for _ in range(3):
                c()
        torch.cuda.synchronize()
        one = max(abtime.timed(stream, c, 1) for c in calls.values())
        reps = max(1, min(200, int(5.0 / max(one, 1e-3))))
        times = abtime.alternate(stream, calls, warmup=0, rounds=5, reps=reps)  # (warmed up above)
    return times


def line(head, times, nbytes, base=None):
    md = {k: float(np.median(v)) for k, v in times.items()}
    out = head
    for k, v in times.items():
        out += f" | {k} {abtime.cell(v)} {nbytes / (md[k] * 1e-3) / 8e12:.3f}"
    if base:
        out += " | vs per-level:" + "".join(f" {k} {md[base] / md[k]:.2f}x" for k in md if k != base)
    return out


ctxs = {"fused": ctx(2), "per-level": ctx(0), "default": ctx(1)}
print("shares of 8 TB/s at 8 bytes per input point", flush=True)
for n in [int(a) for a in sys.argv[1:]] or [1024, 2048, 4096, 8192, 16384]:
    rows = (64 << 20) // n
    x = torch.empty((rows, n), dtype=torch.float32, device="cuda").uniform_(-1, 1)
    a = torch.empty(rows * n, dtype=torch.float32, device="cuda")
    d = torch.empty(rows * n, dtype=torch.float32, device="cuda")
    y = torch.empty_like(x)
    nbytes = 8 * rows * n
    for name in NAMES:
        f = ctxs["default"]
        t = measure({"fwd": lambda: f.dwt_dev(name, x.data_ptr(), a.data_ptr(), d.data_ptr(), n, rows),
                     "inv": lambda: f.idwt_dev(name, a.data_ptr(), d.data_ptr(), y.data_ptr(), n // 2, rows)})
        print(line(f"{name:5s} n {n:6d} rows {rows:7d} single-level:", t, nbytes), flush=True)
        for levels in (1, 2, 3, 5, 8):
            lens = kofft_amd.api.dwt_multi_lengths(n, levels)
            t = measure({k: (lambda c=c: c.wavedec_dev(name, x.data_ptr(), a.data_ptr(), d.data_ptr(), n, rows, levels))
                         for k, c in ctxs.items()})
            print(line(f"{name:5s} n {n:6d} rows {rows:7d} wavedec L={levels}:", t, nbytes, "per-level"), flush=True)
            t = measure({k: (lambda c=c: c.waverec_dev(name, a.data_ptr(), d.data_ptr(), lens[1:], y.data_ptr(), lens[-1], rows))
                         for k, c in ctxs.items()})
            print(line(f"{name:5s} n {n:6d} rows {rows:7d} waverec L={levels}:", t, nbytes, "per-level"), flush=True)
    del x, a, d, y
    torch.cuda.empty_cache()
