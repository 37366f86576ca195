"""Welch power spectra and cross spectra of rows on device memory, HIP events.  In one process a set_welch_fused(2)
context (the fused kernel) alternates with a set_welch_fused(0) context (one-sided frames into the scratch, then the sums), with the
default context (mode 1, the shipped rule) and with what a caller ran on the device without these entry points: stft_onesided_dev into
a buffer of rows x frames x (win_len / 2 + 1) complex values they own, then a torch reduction of re^2 + im^2 over the frames.  `frames`
is the number of whole segments.  Three warm-up calls, then five rounds of 10 timed calls each, the routes alternating; median
[min .. max] ms per call.  Each shape is followed by one line for the cross spectrum of two such batches (no by-hand chain).
usage: bench_welch.py [rows len win_len hop ...]      (groups of four; none: the shapes of DESIGN.md 5.26)"""
import sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime
ctxs = {"fused": kofft_amd.HipFftImpl(np.float32), "composed": kofft_amd.HipFftImpl(np.float32), "default": kofft_amd.HipFftImpl(np.float32)}
ctxs["fused"].set_welch_fused(2)
ctxs["composed"].set_welch_fused(0)
stream = abtime.one_stream(*ctxs.values())


def run(calls, head):
    with torch.cuda.stream(stream):
        times = abtime.alternate(stream, calls, warmup=3, rounds=5, reps=10)
    line = head
    for k, t in times.items():
        line += f" | {k} {abtime.cell(t)}"
    print(line, flush=True)


args = [int(a) for a in sys.argv[1:]]
shapes = [tuple(args[i:i + 4]) for i in range(0, len(args), 4)] or [(1, 28_800_000, 1024, 256), (4096, 16000, 512, 256),
                                                                     (64, 480_000, 2048, 1024), (1024, 16384, 256, 128)]
for rows, length, win_len, hop in shapes:
    frames, K = (length - win_len) // hop + 1, win_len // 2 + 1
    with torch.cuda.stream(stream):
        x = torch.empty((rows, length), dtype=torch.float32, device="cuda").normal_()
        y = torch.empty((rows, length), dtype=torch.float32, device="cuda").normal_()
        win = torch.hann_window(win_len, periodic=False, dtype=torch.float32, device="cuda")
        out = torch.empty((rows, K), dtype=torch.float32, device="cuda")
        cout = torch.empty((rows, K), dtype=torch.complex64, device="cuda")
        spec = torch.empty((rows, frames, K), dtype=torch.complex64, device="cuda")
    scale = 1.0 / frames

    def chain():
        ctxs["default"].stft_onesided_dev(x.data_ptr(), rows, length, length, win.data_ptr(), win_len, hop, spec.data_ptr(), frames)
        torch.sum(torch.view_as_real(spec).square(), dim=(1, 3), out=out)
        out.mul_(scale)

    welch = {k: (lambda f=f: f.welch_rows_dev(x.data_ptr(), rows, length, length, win.data_ptr(), win_len, hop, frames, out.data_ptr(), scale))
             for k, f in ctxs.items()}
    welch["by hand"] = chain
    run(welch, f"welch rows {rows:5d} len {length:9d} win_len {win_len:5d} hop {hop:5d} frames {frames:7d}:")
    csd = {k: (lambda f=f: f.csd_rows_dev(x.data_ptr(), y.data_ptr(), rows, length, length, win.data_ptr(), win_len, hop, frames,
                                          cout.data_ptr(), scale)) for k, f in ctxs.items()}
    run(csd, f"csd   rows {rows:5d} len {length:9d} win_len {win_len:5d} hop {hop:5d} frames {frames:7d}:")
    del x, y, out, cout, spec
    torch.cuda.empty_cache()
