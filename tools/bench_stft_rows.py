"""STFT, stft_magnitudes and ISTFT over rows of signals on device memory, HIP events.  In one process three things
alternate: (a) the rows call, (b) the loop of the single-signal device call over the rows -- the only way before the rows entries, and
unchanged by them -- and (c) the single-signal call on ONE signal of rows * len samples, the ceiling.  Five rounds of timed windows of
at least 30 ms each (as many calls as a probe after the 2 warm-up calls says that takes, never fewer than 3); median [min .. max] ms per
call.  Fraction of the roofline: 8 TB/s on 4 bytes per sample plus 8 bytes per output point (magnitudes: 4 bytes per kept bin).
ISTFT (mode 1) inverse-transforms its frames in place, so over the repeated calls the frames decay towards zero: the kernels have no
data-dependent path and f32 denormals run at full rate here, so the times stand, but the values mean nothing.
usage: bench_stft_rows.py [stft|mags|istft ...] [--shape ROWS,LEN,WIN,HOP ...]   (--shape replaces the built-in shapes)"""
import sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime
fft = kofft_amd.HipFftImpl(np.float32)
stream = abtime.one_stream(fft)
SHAPES = [(4096, 16000, 512, 128), (256, 480000, 1024, 256), (256, 480000, 400, 160), (8, 28800000 // 8, 1024, 256)]


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
    print(line, flush=True)


def bench(kind, rows, length, win_len, hop):
    frames = -(-length // hop)
    x = torch.empty((rows, length), dtype=torch.float32, device="cuda").uniform_(-1, 1)
    win = torch.from_numpy(kofft_amd.hann(win_len)).cuda()
    one_frames = -(-(rows * length) // hop)
    name = f"{kind:5s} {rows} x {length} win {win_len} hop {hop}"
    if kind == "stft":
        out = torch.empty((max(rows * frames, one_frames), win_len, 2), dtype=torch.float32, device="cuda")
        p, o, w = x.data_ptr(), out.data_ptr(), win.data_ptr()
        calls = {"rows": lambda: fft.stft_rows_dev(p, rows, length, length, w, win_len, hop, o, frames),
                 "loop": lambda: [fft.stft_dev(p + 4 * r * length, length, w, win_len, hop, o + 8 * r * frames * win_len, 0, frames) for r in range(rows)],
                 "one": lambda: fft.stft_dev(p, rows * length, w, win_len, hop, o, 0, one_frames)}
        run(name, calls, 4 * rows * length + 8 * rows * frames * win_len)
    elif kind == "mags":
        half = win_len // 2
        out = torch.empty((max(rows * frames, one_frames), half), dtype=torch.float32, device="cuda")
        mx = torch.empty(rows, dtype=torch.float32, device="cuda")
        p, o, m = x.data_ptr(), out.data_ptr(), mx.data_ptr()
        calls = {"rows": lambda: fft.stft_magnitudes_rows_dev(p, rows, length, length, win_len, hop, o, frames, m),
                 "loop": lambda: [fft.stft_magnitudes_dev(p + 4 * r * length, length, win_len, hop, o + 4 * r * frames * half, frames, m + 4 * r)
                                  for r in range(rows)],
                 "one": lambda: fft.stft_magnitudes_dev(p, rows * length, win_len, hop, o, one_frames, m)}
        run(name, calls, 4 * rows * length + 4 * rows * frames * half)
    else:
        spec = torch.empty((rows * frames, win_len, 2), dtype=torch.float32, device="cuda").uniform_(-1, 1)
        out = torch.zeros((rows, length), dtype=torch.float32, device="cuda")
        scr = torch.zeros((rows, length), dtype=torch.float32, device="cuda")
        s, o, c, w = spec.data_ptr(), out.data_ptr(), scr.data_ptr(), win.data_ptr()
        calls = {"rows": lambda: fft.istft_rows_dev(s, rows, frames, w, win_len, hop, o, length, c),
                 "loop": lambda: [fft.istft_dev(s + 8 * r * frames * win_len, frames, w, win_len, hop, o + 4 * r * length, length, c + 4 * r * length)
                                  for r in range(rows)]}
        run(name, calls, 8 * rows * frames * win_len + 8 * rows * length)


args, custom = sys.argv[1:], []
while "--shape" in args:
    i = args.index("--shape")
    custom.append(tuple(int(v) for v in args[i + 1].split(",")))
    del args[i:i + 2]
for kind in args or ["stft", "mags", "istft"]:
    for shape in custom or (SHAPES[:2] if kind == "istft" else SHAPES):
        bench(kind, *shape)
