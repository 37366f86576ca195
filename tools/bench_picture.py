"""Rows of audio to spectrogram pictures on device memory (kofft_hip_dev_stft_picture_f32), HIP events, one process.  Routes,
alternating: the CHAIN -- the calls a caller made before this entry existed, stft_magnitudes_rows_dev into a caller-owned magnitudes
buffer, then one spectrogram_render_dev per row: the yardstick (3 channels only: the render has no RGBA) --, and the one call with
max_mode 0 (the row's maximum), 1 (the running maximum) and 2 (given: the chain's maxima), at 3 and at 4 channels; "row/64M" is
max_mode 0 on a context created under KOFFT_HIP_SCRATCH_CHUNK_MB=64, where the large shapes take the two-pass route (a max-only pass
of the magnitudes kernels, then chunk after chunk).  Before timing, max_mode 0 and 2 at 3 channels are compared with the chain's bytes.
Five rounds of 10 timed calls each, after 3 warm-up calls; median [min .. max] ms per call.
Shapes (rows, len, win_len, hop): config 4's stream, 64 clips of ten seconds at 2048 / 512, 1024 clips of 16 384 samples at 256 / 64.
usage: bench_picture.py [shape index | rows,len,win_len,hop ...]   (every shape in layout image and frames)"""
import os, sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import ctypes as C
import numpy as np, torch, kofft_amd, abtime
SHAPES = [(1, 28_800_000, 1024, 256), (64, 480_000, 2048, 512), (1024, 16_384, 256, 64)]
ctx = {"chain": kofft_amd.HipFftImpl(np.float32), "one": kofft_amd.HipFftImpl(np.float32)}
os.environ["KOFFT_HIP_SCRATCH_CHUNK_MB"] = "64"
ctx["64M"] = kofft_amd.HipFftImpl(np.float32)
del os.environ["KOFFT_HIP_SCRATCH_CHUNK_MB"]
stream = abtime.one_stream(*ctx.values())


for arg in sys.argv[1:] or range(len(SHAPES)):
    rows, length, win_len, hop = [int(v) for v in arg.split(",")] if "," in str(arg) else SHAPES[int(arg)]
    frames, bins = -(-length // hop), win_len // 2
    x = torch.empty((rows, length), dtype=torch.float32, device="cuda").normal_()
    mags = torch.empty((rows, frames, bins), dtype=torch.float32, device="cuda")
    mx = torch.empty((rows,), dtype=torch.float32, device="cuda")
    mo = torch.empty((rows,), dtype=torch.float32, device="cuda")
    pic = {k: torch.empty((rows, frames * bins * 4), dtype=torch.uint8, device="cuda") for k in ("chain", "one")}
    for layout, lname in ((1, "image"), (0, "frames")):
        def chain():
            f = ctx["chain"]
            f.stft_magnitudes_rows_dev(x.data_ptr(), rows, length, length, win_len, hop, mags.data_ptr(), frames, mx.data_ptr())
            for r in range(rows):
                f._lib.kofft_hip_dev_spectrogram_render_f32(f._ctx, C.c_void_p(mags[r].data_ptr()), frames, bins, C.c_void_p(mx[r].data_ptr()), 0, -80.0,
                                                            6, 8, 0, layout, None, C.c_void_p(pic["chain"].data_ptr() + r * frames * bins * 3))

        def one(name, max_mode, channels):
            f = ctx[name]
            return lambda: f.stft_picture_rows_dev(x.data_ptr(), rows, length, length, 0, win_len, hop, frames, max_mode, mx.data_ptr(), mo.data_ptr(), 0,
                                                   -80.0, 6, 8, channels, 0, layout, None, pic["one"].data_ptr())

        calls = {"chain": chain, "row/3": one("one", 0, 3), "given/3": one("one", 2, 3), "running/3": one("one", 1, 3), "row/4": one("one", 0, 4),
                 "given/4": one("one", 2, 4), "running/4": one("one", 1, 4), "row/64M/3": one("64M", 0, 3)}
        times = {k: [] for k in calls}
        nb = rows * frames * bins * 3
        with torch.cuda.stream(stream):
            for c in calls.values():
                for _ in range(3):
                    c()
            torch.cuda.synchronize()
            same = {}
            for k in ("row/3", "given/3", "row/64M/3"):
                calls[k](); torch.cuda.synchronize()
                same[k] = torch.equal(pic["one"].view(-1)[:nb], pic["chain"].view(-1)[:nb])
            for _ in range(5):
                for k, c in calls.items():
                    times[k].append(abtime.timed(stream, c))
        line = f"rows {rows:5d} len {length:9d} win {win_len:5d} hop {hop:4d} layout {lname:6s} frames {rows * frames:8d} == chain: {same}:"
        for k, t in times.items():
            line += f" | {k} {abtime.cell(t)}"
        print(line, flush=True)
    del x, mags, mx, mo, pic
    torch.cuda.empty_cache()
