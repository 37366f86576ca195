"""czt::czt_f32 and goertzel::goertzel_f32 on device memory, HIP events, one process, the variants alternating on the
same buffers; five rounds after 3 warm-up calls, median [min .. max] ms per call.
 * czt table: route 2 (cached table + the direct kernels) at (n, 2m) = (256, 256), (1024, 1024), (4096, 4096), rows as
   bench_trig_direct.py takes them, beside kofft_hip_dct_direct_f32 DCT-II at the same n and rows (the same kernel, the same tile
   count): T terms / s of both and their ratio.  The table build per (n, m): a batch-1 call on a context whose table was just
   dropped (release_scratch) minus the same call with the table cached, HIP events (the kernel and its sums) and the host clock
   (hipMalloc and the pows upload as well), median of five.
 * czt sum: route 1 against route 2 with a cached table and against a fresh table per call (a new context each time), at batch 1, 4,
   16, 64: what czt_use_table() is set from.
 * goertzel: n = 4096, nfreq 1 and 8, rows x nfreq = 524288 lanes (256 CUs x 4 SIMDs x 3 waves x 64 lanes = 196608 fill the device at
   the kernel's 136 VGPRs): GB/s of input read, beside a device-to-device copy of the same bytes.
usage: bench_spectral.py [table] [sum] [goertzel]"""
import sys, pathlib, time; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime

stream = abtime.one_stream()
W = lambda m: np.exp(-2j * np.pi / m)
A = np.exp(2j * np.pi * 0.1)


def ctx(route=0):
    f = kofft_amd.HipFftImpl(np.float32)
    f.set_czt_route(route)
    f.set_stream(stream.cuda_stream)
    return f


def rounds(calls, warm=3, n=5, budget_ms=5.0):
    with torch.cuda.stream(stream):
        for c in calls.values():
            for _ in range(warm):
                c()
        torch.cuda.synchronize()
        one = max(abtime.timed(stream, c, 1) for c in calls.values())
        reps = max(1, min(50, int(budget_ms / max(one, 1e-3))))
        times = abtime.alternate(stream, calls, warmup=0, rounds=n, reps=reps)  # (warmed up above)
    return {k: (float(np.median(t)), min(t), max(t)) for k, t in times.items()}


def fmt(t):
    return f"{t[0]:.3f} ms [{t[1]:.3f} .. {t[2]:.3f}]"


def bench_table():
    tab, dct = ctx(2), ctx(0)
    for n in (256, 1024, 4096):
        m = n // 2
        rows = int(min(max(3e10 // (n * n), 64), (64 << 20) // n))
        x = torch.empty((rows, n), dtype=torch.float32, device="cuda").uniform_(-1, 1)
        y = torch.empty((rows, 2 * m), dtype=torch.float32, device="cuda")
        build_ev, build_host = [], []
        with torch.cuda.stream(stream):
            one = lambda: tab.czt_dev(x.data_ptr(), y.data_ptr(), n, m, W(m), A, 1)
            for _ in range(5):
                tab.release_scratch()  # drops the table: the next call builds it
                torch.cuda.synchronize(); t0 = time.perf_counter(); ev = abtime.timed(stream, one, 1); host = (time.perf_counter() - t0) * 1e3
                torch.cuda.synchronize(); t0 = time.perf_counter(); ev1 = abtime.timed(stream, one, 1); host1 = (time.perf_counter() - t0) * 1e3
                build_ev.append(ev - ev1); build_host.append(host - host1)
        r = rounds({"czt": lambda: tab.czt_dev(x.data_ptr(), y.data_ptr(), n, m, W(m), A, rows),
                    "dct2": lambda: dct.dct_direct_dev(2, x.data_ptr(), y.data_ptr(), n, rows)})
        terms = rows * n * 2 * m
        print(f"czt table n {n} 2m {2 * m} rows {rows} table build {float(np.median(build_ev)):.3f} ms on the device, "
              f"{float(np.median(build_host)):.3f} ms on the host clock | czt {fmt(r['czt'])} {terms / r['czt'][0] / 1e9:.2f} Tterm/s"
              f" | dct2 {fmt(r['dct2'])} {terms / r['dct2'][0] / 1e9:.2f} Tterm/s | czt / dct2 rate {r['dct2'][0] / r['czt'][0]:.3f}", flush=True)
        tab.release_scratch()
        del x, y
        torch.cuda.empty_cache()


def bench_sum():
    summ, tab = ctx(1), ctx(2)
    for n, m in ((64, 64), (256, 256), (1024, 1024), (4096, 4096)):
        for batch in (1, 4, 16, 64):
            x = torch.empty((batch, n), dtype=torch.float32, device="cuda").uniform_(-1, 1)
            y = torch.empty((batch, 2 * m), dtype=torch.float32, device="cuda")

            def fresh_table():
                f = ctx(2)
                f.czt_dev(x.data_ptr(), y.data_ptr(), n, m, W(m), A, batch)
                f.synchronize()

            r = rounds({"sum": lambda: summ.czt_dev(x.data_ptr(), y.data_ptr(), n, m, W(m), A, batch),
                        "cached": lambda: tab.czt_dev(x.data_ptr(), y.data_ptr(), n, m, W(m), A, batch)})
            host = []
            for _ in range(3):  # a context, the pows upload, hipMalloc, the table kernel and the sums, on the host clock
                torch.cuda.synchronize(); t0 = time.perf_counter(); fresh_table(); host.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); c0 = ctx(2); c0.synchronize(); ctx_ms = (time.perf_counter() - t0) * 1e3; del c0
            print(f"czt sum n {n} m {m} batch {batch}: sum {fmt(r['sum'])} | cached table {fmt(r['cached'])} | fresh table, host clock "
                  f"{float(np.median(host)):.3f} ms of which a new context {ctx_ms:.3f} ms", flush=True)
        tab.release_scratch()


def bench_goertzel():
    f = ctx()
    n = 4096
    for nfreq in (1, 8):
        rows = 524288 // nfreq  # nfreq 1: 8 GiB of input, nfreq 8: 1 GiB
        x = torch.empty((rows, n), dtype=torch.float32, device="cuda").uniform_(-1, 1)
        x2 = torch.empty_like(x)
        freqs = np.linspace(100.0, 3900.0, nfreq).astype(np.float32)
        y = torch.empty((rows, nfreq), dtype=torch.float32, device="cuda")
        r = rounds({"goertzel": lambda: f.goertzel_dev(x.data_ptr(), y.data_ptr(), n, rows, 8000.0, freqs),
                    "copy": lambda: x2.copy_(x)}, budget_ms=20.0)
        gb = 4 * rows * n / 1e9
        print(f"goertzel n {n} rows {rows} nfreq {nfreq}: {fmt(r['goertzel'])} {gb / r['goertzel'][0] * 1e3:.0f} GB/s read | copy {fmt(r['copy'])} "
              f"{gb / r['copy'][0] * 1e3:.0f} GB/s read (+ as much written) | goertzel / copy time {r['goertzel'][0] / r['copy'][0]:.2f}", flush=True)
        del x, x2, y
        torch.cuda.empty_cache()


which = sys.argv[1:] or ["table", "sum", "goertzel"]
for name in which:
    {"table": bench_table, "sum": bench_sum, "goertzel": bench_goertzel}[name]()
