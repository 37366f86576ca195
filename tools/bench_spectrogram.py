"""The spectrogram render on device memory at config 4's magnitudes: 28.8 M samples, win 1024, hop 256 = 112500 frames x
512 bins, Fire, depth 8, floor -120 dB, HIP events on one stream, one process.  The magnitudes and their maximum come from
stft_magnitudes_rows_dev, whose time for the same frames is the yardstick.  Timed: linear / log x frame-major / image on the default
context (the image layout through the LDS exchange), and the image layout on a set_transpose(False) context (every lane stores its
own bytes), the two alternating round by round.  Before timing, the two image results are compared byte for byte.  Rounds of 10 timed
calls each after 3 warm-up calls (50 timed launches per entry); median [min .. max] ms per call and the fraction of 8 TB/s on 7 bytes
per pixel (4 in, 3 out).
usage: bench_spectrogram.py [frames [bins [rounds]]]"""
import sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime
from kofft_amd import spectrogram as sp
frames = int(sys.argv[1]) if len(sys.argv) > 1 else 112500
bins = int(sys.argv[2]) if len(sys.argv) > 2 else 512
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
win, hop = 2 * bins, bins // 2
length = frames * hop
lds = kofft_amd.HipFftImpl(np.float32)
direct = kofft_amd.HipFftImpl(np.float32)
sp.set_transpose(False, fft=direct)
stream = abtime.one_stream(lds, direct)
sig = torch.empty(length, dtype=torch.float32, device="cuda").uniform_(-1, 1)
mags = torch.empty((frames, bins), dtype=torch.float32, device="cuda")
d_max = torch.zeros(1, dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
outs = {}


def render(f, key, scale, layout):
    def call():
        outs[key] = sp.render(mags, d_max, 0, -120.0, "fire", 8, scale, layout, fft=f)
    return call


calls = {"stft_magnitudes_rows": lambda: lds.stft_magnitudes_rows_dev(sig.data_ptr(), 1, length, length, win, hop, mags.data_ptr(), frames, d_max.data_ptr()),
         "linear frame-major": render(lds, "lf", "linear", "frames"), "log frame-major": render(lds, "gf", "log", "frames"),
         "linear image LDS": render(lds, "li", "linear", "image"), "linear image direct": render(direct, "di", "linear", "image"),
         "log image LDS": render(lds, "gi", "log", "image"), "log image direct": render(direct, "dgi", "log", "image")}
times = {k: [] for k in calls}
with torch.cuda.stream(stream):
    for c in calls.values():
        for _ in range(3):
            c()
    torch.cuda.synchronize()
    same = torch.equal(outs["li"], outs["di"]) and torch.equal(outs["gi"], outs["dgi"])
    flipped = torch.equal(outs["li"], torch.flip(outs["lf"], dims=(1,)).transpose(0, 1))
    for _ in range(rounds):
        for k, c in calls.items():
            times[k].append(abtime.timed(stream, c))
print(f"frames {frames} bins {bins}: LDS == direct: {same}; image == flipped transpose of frame-major: {flipped}; max_mag {float(d_max[0]):.4f}")
for k, t in times.items():
    md = float(np.median(t))
    frac = 7 * frames * bins / (md * 1e-3) / 8e12
    print(f"  {k:22s} {md:8.3f} ms [{min(t):.3f} .. {max(t):.3f}]" + ("" if k.startswith("stft") else f"  {frac:.3f} of 8 TB/s"), flush=True)
