"""The A/B protocol of the family benchmarks (tools/bench_*.py), the one by which default routes are decided: every candidate's
contexts on ONE torch stream, the candidates ALTERNATING in one process -- the warm-up calls of every candidate first, then rounds
in which each candidate is timed once, in the same order every round -- and a cell of "median ms [min .. max]" per candidate.  A
tool keeps its own shapes, warm-up count, rounds and repetitions and passes them in.  torch is imported inside the functions: the
module loads (and tests/test_abtime_cpu.py runs) on a machine without a GPU."""
import statistics


def one_stream(*contexts):
    """A new torch stream with every context (kofft_amd.HipFftImpl) put on it."""
    import torch
    stream = torch.cuda.Stream()
    for f in contexts:
        f.set_stream(stream.cuda_stream)
    return stream


def timed(stream, call, reps=10):
    """ms per call of `reps` back-to-back calls, by HIP events on `stream`."""
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record(stream)
    for _ in range(reps):
        call()
    e.record(stream); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def alternate(stream, calls, warmup=3, rounds=5, reps=10, timer=timed):
    """calls: {name: callable}.  `warmup` untimed calls of every candidate, the stream drained, then `rounds` rounds of one
    timer(stream, call, reps) per candidate in the dict's order.  reps: one count, or {name: count}.  -> {name: [ms per call]}"""
    for c in calls.values():
        for _ in range(warmup):
            c()
    stream.synchronize()
    times = {k: [] for k in calls}
    for _ in range(rounds):
        for k, c in calls.items():
            times[k].append(timer(stream, c, reps[k] if isinstance(reps, dict) else reps))
    return times


def cell(ms):
    """'median ms [min .. max]' of a candidate's timings."""
    return f"{statistics.median(ms):.3f} ms [{min(ms):.3f} .. {max(ms):.3f}]"
