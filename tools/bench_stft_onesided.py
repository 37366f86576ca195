"""The one-sided STFT over rows of signals and its inverse on device memory, HIP events.  In one process three forms
alternate: (a) `onesided`, the one-sided call; (b) `rows`, kofft_hip_dev_stft_rows_f32 on the same input (all win_len bins); (c)
`rows+slice`, that call followed by a torch slice-and-contiguous() to K = win_len / 2 + 1 bins -- what a caller who wants one side has
to do without (a).  Five rounds of timed windows of at least 30 ms each (as many calls as a probe after the 2 warm-up calls says that
takes, never fewer than 3); median [min .. max] ms per call.  The last figure of each form is the fraction of 8 TB/s on the bytes of the
ONE-SIDED result, 4 * len + 8 * frames * K per row (the same work for all three, so the figures compare); for the inverse, on
8 * frames * K + 8 * len per row (the output is read and written).
Inverse: `onesided` against `parallel`, kofft_hip_dev_istft_parallel_rows_f32 on the completed frames.
usage: bench_stft_onesided.py [stft|istft ...] [--shape ROWS,LEN,WIN,HOP ...]   (--shape replaces the built-in shapes)"""
import sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime
fft = kofft_amd.HipFftImpl(np.float32)
stream = abtime.one_stream(fft)
SHAPES = [(4096, 16000, 512, 128), (256, 480000, 1024, 256), (1, 28800000, 1024, 256), (256, 480000, 400, 160)]


def run(name, calls, nbytes):
    with torch.cuda.stream(stream):
        for c in calls.values():
            for _ in range(2):
                c()
        torch.cuda.synchronize()
        reps = {k: max(3, int(np.ceil(30.0 / max(abtime.timed(stream, c, 2), 1e-3)))) for k, c in calls.items()}  # windows of 30 ms and more
        times = abtime.alternate(stream, calls, warmup=0, rounds=5, reps=reps)  # (warmed up above)
    line = name
    for k, t in times.items():
        med = float(np.median(t))
        line += f" | {k} {med:.3f} [{min(t):.3f} .. {max(t):.3f}] ms {nbytes / (med * 1e-3) / 8e12:.3f}"
    first, second = list(times.values())[:2]
    line += f" | max(a) {'<' if max(first) < min(second) else '>='} min(b)"
    print(line, flush=True)


def bench(kind, rows, length, win_len, hop):
    frames, bins = -(-length // hop), win_len // 2 + 1
    win = torch.from_numpy(kofft_amd.hann(win_len)).cuda()
    name = f"{kind:5s} {rows} x {length} win {win_len} hop {hop}"
    w = win.data_ptr()
    if kind == "stft":
        x = torch.empty((rows, length), dtype=torch.float32, device="cuda").uniform_(-1, 1)
        full = torch.empty((rows * frames, win_len, 2), dtype=torch.float32, device="cuda")
        half = torch.empty((rows * frames, bins, 2), dtype=torch.float32, device="cuda")
        p, o, h = x.data_ptr(), full.data_ptr(), half.data_ptr()

        def rows_then_slice():
            fft.stft_rows_dev(p, rows, length, length, w, win_len, hop, o, frames)
            return full[:, :bins].contiguous()
        calls = {"onesided": lambda: fft.stft_onesided_dev(p, rows, length, length, w, win_len, hop, h, frames),
                 "rows": lambda: fft.stft_rows_dev(p, rows, length, length, w, win_len, hop, o, frames),
                 "rows+slice": rows_then_slice}
        run(name, calls, 4 * rows * length + 8 * rows * frames * bins)
    else:
        half = torch.empty((rows * frames, bins, 2), dtype=torch.float32, device="cuda").uniform_(-1, 1)
        idx = torch.arange(win_len, device="cuda")
        full = torch.where((idx < bins)[None, :, None], half[:, torch.clamp(idx, max=bins - 1)],
                           half[:, torch.clamp(win_len - idx, max=bins - 1)] * torch.tensor([1.0, -1.0], device="cuda")).contiguous()
        out = torch.zeros((rows, length), dtype=torch.float32, device="cuda")
        h, f, o = half.data_ptr(), full.data_ptr(), out.data_ptr()
        calls = {"onesided": lambda: fft.istft_onesided_dev(h, rows, frames, w, win_len, hop, o, length),
                 "parallel": lambda: fft.istft_rows_dev(f, rows, frames, w, win_len, hop, o, length, parallel=True)}
        run(name, calls, 8 * rows * frames * bins + 8 * rows * length)


args, custom = sys.argv[1:], []
while "--shape" in args:
    i = args.index("--shape")
    custom.append(tuple(int(v) for v in args[i + 1].split(",")))
    del args[i:i + 2]
for kind in args or ["stft", "istft"]:
    for shape in custom or (SHAPES[:2] if kind == "istft" else SHAPES):
        bench(kind, *shape)
