"""hartley::dht on device memory, in the manner of tools/bench_trig_direct.py.  Two tables:
(a) the first call of a FRESH context at n = 256, 1024, 4096 on 64 rows, timed from the call to the end of the stream's work by the host's
    clock and by HIP events around the call, with
    the table built on the device (dht_table_kernel) against built on the host and uploaded (set_dht_table_device(False)): the same
    process, the two alternating, medians of 5 after one untimed pair (which pays the code object's load).  The only place the new
    kernel can win or lose.  The steady-state call of the same shape is printed beside it: first-call minus steady-state is the table.
(b) the steady-state ms per call at the DCT-II shapes of DESIGN 5.14's table (n = 32 .. 4096, about 3e10 terms), HIP events, five
    rounds after 3 warm-up calls, median [min .. max], beside the DCT-II of the same context and buffers: the sums run on the direct
    family's kernels, so the two should agree.
usage: bench_hartley.py [first|steady ...]"""
import sys, pathlib, time; sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np, torch, kofft_amd, abtime

CEIL_TERMS = 157.3e12 / 4  # one mul + one add per term
stream = abtime.one_stream()


def ctx(table_device=True):
    f = kofft_amd.HipFftImpl(np.float32)
    f.set_dht_table_device(table_device)
    f.set_stream(stream.cuda_stream)
    return f


def first_call(n, rows, x, y, table_device):
    """(host-clock ms, event ms) of a fresh context's first call: the events bracket the call on the stream, so the device's clock
    sees the host's table build and upload too (the stream is idle meanwhile)."""
    f = ctx(table_device)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s.record(stream)
    f.dht_dev(x.data_ptr(), y.data_ptr(), n, rows)
    e.record(stream)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    f.close()
    return ms, s.elapsed_time(e)


def med(v):
    return f"{float(np.median(v)):8.3f} ms [{min(v):.3f} .. {max(v):.3f}]"


def first_table():
    for n in (256, 1024, 4096):
        rows = 64
        x = torch.empty((rows, n), dtype=torch.float32, device="cuda").uniform_(-1, 1)
        y = torch.empty_like(x)
        with torch.cuda.stream(stream):
            for dev in (True, False):
                first_call(n, rows, x, y, dev)  # untimed: the code object, the allocator
            t = {True: [], False: []}
            for _ in range(5):
                for dev in (True, False):
                    t[dev].append(first_call(n, rows, x, y, dev))
            warm = ctx(True)
            for _ in range(3):
                warm.dht_dev(x.data_ptr(), y.data_ptr(), n, rows)
            steady = float(np.median([abtime.timed(stream, lambda: warm.dht_dev(x.data_ptr(), y.data_ptr(), n, rows), 20) for _ in range(5)]))
            warm.close()
        dh, de = [a for a, _ in t[True]], [b for _, b in t[True]]
        hh, he = [a for a, _ in t[False]], [b for _, b in t[False]]
        print(f"first-call n {n:5d} rows {rows}: device table host-clock {med(dh)} events {med(de)} | host table host-clock {med(hh)} events {med(he)}"
              f" | host / device {np.median(hh) / np.median(dh):.2f} (events {np.median(he) / np.median(de):.2f}) | steady-state {steady:.4f} ms", flush=True)
        del x, y
        torch.cuda.empty_cache()


def steady_table():
    f = ctx(True)
    for n in (32, 64, 256, 1024, 4096):
        rows = int(min(max(3e10 // (n * n), 64), (64 << 20) // n))
        x = torch.empty((rows, n), dtype=torch.float32, device="cuda").uniform_(-1, 1)
        y = torch.empty_like(x)
        terms = rows * n * n
        with torch.cuda.stream(stream):
            calls = {"dht": lambda: f.dht_dev(x.data_ptr(), y.data_ptr(), n, rows),
                     "dct2": lambda: f.dct_direct_dev(2, x.data_ptr(), y.data_ptr(), n, rows)}
            for c in calls.values():
                for _ in range(3):
                    c()
            torch.cuda.synchronize()
            one = max(abtime.timed(stream, c, 1) for c in calls.values())
            reps = max(1, min(50, int(5.0 / max(one, 1e-3))))
            times = abtime.alternate(stream, calls, warmup=0, rounds=5, reps=reps)  # (warmed up above)
        line = f"steady n {n:5d} rows {rows:8d}:"
        for k, t in times.items():
            md = float(np.median(t))
            tps = terms / (md * 1e-3)
            line += f" | {k} {abtime.cell(t)} {tps / 1e12:.2f} Tterm/s valu {tps / CEIL_TERMS:.3f}"
        print(line, flush=True)
        del x, y
        torch.cuda.empty_cache()
    f.close()


for what in sys.argv[1:] or ["first", "steady"]:
    {"first": first_table, "steady": steady_table}[what]()
