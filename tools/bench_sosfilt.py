"""IIR filtering of rows by a cascade of biquads on device memory, HIP events.  In one process a
set_sosfilt_tiled(2) context (the tiled kernel), a set_sosfilt_tiled(0) context (the plain kernel) and the default context alternate
on the same device-resident buffers, out of place, with an initial and a final state.  Three warm-up calls, then five rounds of 10
timed calls each; median [min .. max] ms per call.  A route whose first warm-up call takes longer than 0.2 s is measured with that one
warm-up call and three rounds of one call; one whose warm-up call takes longer than --skip-above seconds (default 3) is not timed
further and its one call is what the line shows.  Fraction of the roofline: 8 TB/s on 8 rows nx bytes (every sample read once and
written once, whatever the number of sections or passes).
usage: bench_sosfilt.py [--skip-above S] [rows nx sections reverse ...]   (groups of four; none: the matrix of DESIGN.md 5.29)"""
import sys, pathlib; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime
argv = sys.argv[1:]
skip_above = 3.0
if argv[:1] == ["--skip-above"]:
    skip_above = float(argv[1])
    argv = argv[2:]
ctxs = {"tiled": kofft_amd.HipFftImpl(np.float32), "plain": kofft_amd.HipFftImpl(np.float32), "default": kofft_amd.HipFftImpl(np.float32)}
ctxs["tiled"].set_sosfilt_tiled(2)
ctxs["plain"].set_sosfilt_tiled(0)
stream = abtime.one_stream(*ctxs.values())


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
    (rows, nx, sections, reverse) for rows, nx in [(65536, 3000), (1 << 20, 200), (4096, 48000), (16, 1 << 24)]
    for sections in (1, 2, 4, 8, 12) for reverse in (0, 1)]
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
    calls = {k: (lambda f=f: f.sosfilt_dev(x.data_ptr(), rows, nx, sos.data_ptr(), sections, zi.data_ptr(), zf.data_ptr(), out.data_ptr(),
                                           reverse=bool(reverse))) for k, f in ctxs.items()}
    times, plan, note = {k: [] for k in calls}, {}, {}
    with torch.cuda.stream(stream):
        for k, c in calls.items():
            first = abtime.timed(stream, c, 1)
            if first > skip_above * 1e3:
                plan[k], note[k] = (0, 0), f"one call {first:.0f} ms, not timed further"
                continue
            slow = first > 200.0
            plan[k] = (3, 1) if slow else (5, 10)
            for _ in range(0 if slow else 2):
                c()
        torch.cuda.synchronize()
        for rnd in range(5):
            for k, c in calls.items():
                if rnd < plan[k][0]:
                    times[k].append(abtime.timed(stream, c, plan[k][1]))
    frac = lambda ms: 8.0 * nx * rows / (ms * 1e-3) / 8e12
    line = f"rows {rows:8d} nx {nx:9d} sections {sections:2d} {'reverse' if reverse else 'forward'}:"
    for k, t in times.items():
        if not t:
            line += f" | {k} {note[k]}"
            continue
        md = float(np.median(t))
        line += f" | {k} {abtime.cell(t)} {frac(md):.4f}"
        if plan[k] != (5, 10):
            line += f" ({plan[k][0]} x {plan[k][1]})"
    print(line, flush=True)
    del sos, zi, zf
