"""IIR filtering of rows as a scan along time against the sequential filter (5.29) on device memory, HIP events.  In
one process, on one default context and the same device-resident buffers, out of place, with an initial and a final state, the
candidates alternate: kofft_hip_dev_sosfilt_f32 (the baseline) and kofft_hip_dev_sosfilt_scan_f32 at every chunk of --chunks.  Three
warm-up calls, then five rounds of 10 timed calls each; median [min .. max] ms per call.  A candidate whose first warm-up call takes
longer than 0.2 s is measured with that one warm-up call and three rounds of one call (5.29's slow-call rule).  Fraction of the
roofline: 8 TB/s on the bytes that candidate moves -- 8 rows nx for the baseline (every sample read once, written once), 12 rows nx
for the scan (read twice, written once); passes of a cascade of more than 8 sections are not counted.
usage: bench_sosfilt_scan.py [--chunks a,b,..] [rows nx sections reverse ...]   (groups of four; none: the matrix of DESIGN.md 5.30)"""
import sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime
argv = sys.argv[1:]
chunks = [1024, 2048, 4096, 8192, 16384]
if argv[:1] == ["--chunks"]:
    chunks = [int(c) for c in argv[1].split(",")]
    argv = argv[2:]
fft = kofft_amd.HipFftImpl(np.float32)
stream = abtime.one_stream(fft)


def cascade(sections):
    """stable biquads: poles of radius 0.5 .. 0.9, the tests' recipe"""
    rng = np.random.default_rng(sections)
    r, th = rng.uniform(0.5, 0.9, sections), rng.uniform(0.2, 2.9, sections)
    sos = np.empty((sections, 6), np.float32)
    sos[:, :3] = rng.uniform(-1, 1, (sections, 3))
    sos[:, 3], sos[:, 4], sos[:, 5] = 1, -2 * r * np.cos(th), r * r
    return sos


args = [int(a) for a in argv]
shapes = [tuple(args[i:i + 4]) for i in range(0, len(args), 4)] or [
    (rows, nx, sections, reverse) for rows, nx in [(1, 28_800_000), (16, 1 << 24), (64, 1 << 20), (4096, 48000), (65536, 3000)]
    for sections in (1, 4, 8, 12) for reverse in (0, 1)]
last = None
for rows, nx, sections, reverse in shapes:
    if last != (rows, nx):
        x = out = None
        torch.cuda.empty_cache()
        x = torch.empty((rows, nx), dtype=torch.float32, device="cuda").uniform_(-1, 1)
        out = torch.empty((rows, nx), dtype=torch.float32, device="cuda")
        last = (rows, nx)
    sos = torch.from_numpy(cascade(sections)).cuda()
    zi = torch.empty((rows, sections, 2), dtype=torch.float32, device="cuda").uniform_(-1, 1)
    zf = torch.empty_like(zi)
    p = (x.data_ptr(), rows, nx, sos.data_ptr(), sections, zi.data_ptr(), zf.data_ptr())
    calls = {"sosfilt": lambda: fft.sosfilt_dev(*p, out.data_ptr(), reverse=bool(reverse))}
    for c in chunks:
        calls[f"scan {c}"] = lambda c=c: fft.sosfilt_scan_dev(*p, c, out.data_ptr(), reverse=bool(reverse))
    times, plan = {k: [] for k in calls}, {}
    with torch.cuda.stream(stream):
        for k, c in calls.items():
            slow = abtime.timed(stream, c, 1) > 200.0
            plan[k] = (3, 1) if slow else (5, 10)
            for _ in range(0 if slow else 2):
                c()
        torch.cuda.synchronize()
        for rnd in range(5):
            for k, c in calls.items():
                if rnd < plan[k][0]:
                    times[k].append(abtime.timed(stream, c, plan[k][1]))
    print(f"rows {rows:6d} nx {nx:9d} sections {sections:2d} {'reverse' if reverse else 'forward'}: recommended chunk "
          f"{kofft_amd.iir.scan_chunk(rows, nx, sections)}", flush=True)
    for k, t in times.items():
        md = float(np.median(t))
        frac = (8.0 if k == "sosfilt" else 12.0) * nx * rows / (md * 1e-3) / 8e12
        line = f"    {k:11s} {md:10.3f} ms [{min(t):.3f} .. {max(t):.3f}] {frac:.5f}"
        if plan[k] != (5, 10):
            line += f" ({plan[k][0]} x {plan[k][1]})"
        print(line, flush=True)
    del sos, zi, zf
