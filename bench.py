#!/usr/bin/env python3
"""bench.py -- headline benchmark of the hot path (BASELINE.json): batched 4096-point Complex32 FFT.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Both forms run N ranks, one per GPU.  Without WORLD_SIZE in the environment and with --gpus N > 1 this
script is the launcher: BEFORE importing torch or touching the GPU it starts N fresh child processes of
itself (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT set), waits for them, relays rank 0's
JSON line and exits non-zero if any child failed.  Nothing is ever exec'ed from a process that has
initialised the GPU.

A "step" is one pass of the hot path over one batch: every rank transforms its own 65 536 x 4096
c32 batch (BASELINE config #2, 2 GiB, resident in HBM) IN PLACE -- the form FftImpl::fft(&mut [Complex<T>])
is (fft.rs:1054; SURVEY 8d states config #2 in place).  Repeated forward transforms grow the values by
sqrt(n) = 64 per step, so before every K-step block the buffer is restored (untimed) to 1e-18 x the
pristine uniform(-1, 1) batch: 64^30 x 1e-18 is still a normal f32, and no step ever computes on inf / NaN.
The out-of-place twin (pristine -> second buffer, rounds 1-4's headline) is measured beside it with the same
protocol and reported as `roofline.configs["#2_oop"]`.  Batches shard across ranks with no data-path
collective (weak scaling); the only collectives are the barriers of the timing protocol and a MAX over ranks
of the elapsed time.

Timing: W warm-up steps, then blocks of EXACTLY K steps, each block bracketed by barrier +
torch.cuda.synchronize() on both sides and reduced with MAX over ranks.  One block is the contract: by
default the headline runs exactly K timed steps and `ms_per_step` is that block's time / K.  With
--min-seconds S > 0 the block is repeated until S seconds of timed work have run (so that utilisation
sampling from outside sees a busy GPU) and the line reports the MEDIAN block (`blocks_ms_per_step` lists the first eight).

--dump-outputs DIR: after the timed steps, what the headline's last step computed (the arrays its caller receives) is
written as DIR/<name>.npy, float32 / float64, at most DUMP_BYTES in all (a fixed, seeded sample of rows of a larger
output).  Inputs are generated from fixed seeds and every block starts from the same pristine state, so two builds run
with the same arguments can be compared output for output.

ONE JSON line is printed by rank 0, kept under ~6 KB so that it survives the driver's tail buffer.  Every BASELINE
config and SURVEY 8(f) row measured in the same processes with the same protocol is summarised inside
`roofline.configs` ("#2_inplace", "#2_oop", "#3", "#4", "#5" with its two-pass cap, "f1" .. "f4": value, ms, frac,
traffic_ratio) and `workloads` (value / unit / ms_per_step / frac per workload); the full per-workload objects
(every roofline field, block lists, shard timings) go to gpurun_out/bench_detail_n<N>.json and to stderr.
At N > 1: config #4 sharded by frames with its RCCL all-gather timed apart, #3 / #5 sharded by batch, no
collective; then rank 0 alone runs config #4 once through the single-process multi-device handle in both gather
modes (`multi_single_process`: RCCL against direct peer copies).  `cpu_baseline`: rank 0's host cores.
See DESIGN.md "Measurement" for how each field is produced.  torch is plumbing only (device memory,
streams, torch.distributed); the transform is libkofft_hip.so.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import threading
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec per GPU

WORKLOADS = {
    "fft4096": "batched 65536 x 4096-pt Complex32 forward FFT (BASELINE config #2)",
    "rfft2048": "batched 2^20 x 2048-pt f32 rfft + Hann (BASELINE config #3)",
    "stft1024": "STFT 28.8M-sample f32 stream, 1024-pt Hann, hop 256 (BASELINE config #4, frames sharded)",
    "c64_2p20": "batched 1024 x 2^20-pt Complex64 forward FFT (BASELINE config #5)",
    # built, parity-tested; measured here with the same protocol (N = 1)
    "istft1024": "ISTFT of config #4's spectra: 112500 x 1024-pt frames, Hann, hop 256 (stft.rs:117-156, 8f row 1)",
    "magnitudes1024": "stft_magnitudes of config #4's stream: 1024-pt Hann, hop 256 (visual/spectrogram.rs:52-76, 8f row 2)",
    "fft2d_4096": "fft2d_inplace of one 4096 x 4096 Complex32 image (ndfft.rs:74-101, 8f row 3)",
    "bluestein1000": "batched 65536 x 1000-pt Complex32 forward FFT, Bluestein arm (fft.rs:1088-1132, 8f row 4)",
}
F_ROWS = ("istft1024", "magnitudes1024", "fft2d_4096", "bluestein1000")
CONFIG_KEY = {"fft4096": "#2", "rfft2048": "#3", "stft1024": "#4", "c64_2p20": "#5",
              "istft1024": "f1", "magnitudes1024": "f2", "fft2d_4096": "f3", "bluestein1000": "f4"}
INPLACE_SCALE = 1e-18        # the in-place batch starts at 1e-18 x uniform(-1, 1) ...
INPLACE_MAX_STEPS = 30       # ... and is restored at the latest after this many forward steps (64^30 x 1e-18 = 1.5e36)
LINE_BUDGET = 6000           # bytes of the JSON line the driver's tail buffer is known to keep
DUMP_BYTES = 48 << 20        # --dump-outputs: array data written in all (under 64 MB with the .npy headers)
DUMP_SEED = 0x6B6F666674     # --dump-outputs: which rows of a larger output are written


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ramp-ms", type=float, default=300.0,
                    help="untimed pre-warm-up: keep the GPU busy this long so DVFS has left idle clocks "
                         "(measured: per-launch time falls 1.17 -> 0.81 ms over the first ~40 ms of load)")
    ap.add_argument("--workload", default="fft4096", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=0, help="override per-GPU batch (debug only; invalidates the metric)")
    ap.add_argument("--min-seconds", type=float, default=0.0,
                    help="repeat the K-step block until this much timed work has run (default 0: exactly one block, K timed steps)")
    ap.add_argument("--all-workloads", dest="extras", action="store_true", default=None,
                    help="also measure the other BASELINE configs into `workloads` (default at --workload fft4096)")
    ap.add_argument("--no-extra-workloads", dest="extras", action="store_false")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--form", choices=("inplace", "oop"), default="inplace",
                    help="fft4096 only: the headline form.  inplace = FftImpl::fft(&mut buf), the API form (default); oop = pristine "
                         "input -> second buffer (the headline of rounds 1-4; now the twin reported in roofline.configs)")
    ap.add_argument("--no-twin", action="store_true", help="fft4096: do not measure the other form beside the headline")
    ap.add_argument("--no-multi-ab", action="store_true", help="N > 1: skip rank 0's single-process RCCL-vs-direct gather A/B of config #4")
    ap.add_argument("--detail-file", default=None, help="where the full per-workload objects go (default gpurun_out/bench_detail_n<N>.json)")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="target CPU work for the cpu_baseline sample")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the headline's last step computed as DIR/<name>.npy (float32 / float64; "
                         "a fixed, seeded sample of rows where the output exceeds the dump budget)")
    ap.add_argument("--extras-timeout", type=float, default=None,
                    help="seconds the extra workloads may take before rank 0 prints the headline alone and exits "
                         "(0 = no limit; default 240 at N > 1, where a hanging collective cannot be caught, none at N = 1)")
    ap.add_argument("--rehearse-one-card", action="store_true",
                    help="rehearsal only (invalidates the metric): every rank uses cuda:0 and the process group is gloo, so the "
                         "N-rank protocol (launcher, barriers, reductions, sharding, gather) can run on a one-GPU box")
    ap.add_argument("--dry-launch", action="store_true",
                    help="launcher self-test: every rank prints its rendezvous environment and exits without touching a GPU")
    ap.add_argument("--dry-protocol", action="store_true",
                    help="with --dry-launch: the ranks also rendezvous (gloo, CPU), run the barrier / all-reduce steps of the timing "
                         "protocol, and rank 0 prints ONE line with the real line's keys (values null): the N-rank contract without a GPU")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


# ---------------------------------------------------------------------------------------------------
# launcher: `python bench.py --gpus N` with no WORLD_SIZE starts the N ranks itself
# ---------------------------------------------------------------------------------------------------
RANK_ENV = ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")


def free_port() -> int:
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return int(s.getsockname()[1])


def profiler_preloaded() -> str | None:
    """Name of the environment entry that shows a GPU profiler has been preloaded into this process, or None.

    rocprofv3 (always with --pmc) initialises the GPU from its preloaded library before Python starts, so this process
    must not start another program: on this pool an exec from a GPU-initialised process takes the machine down."""
    for key, val in os.environ.items():
        low = (key + "=" + val).lower()
        if key == "LD_PRELOAD" and any(t in low for t in ("rocprof", "roctracer", "roctx", "rocprofiler")):
            return f"LD_PRELOAD={val}"
        if key.startswith(("ROCP_", "ROCPROF", "ROCPROFILER", "ROCTRACER", "HSA_TOOLS_LIB")):
            return f"{key}={val}"
    return None


def csrc_sha16() -> str:
    """Hash of the kernel sources: profiles/traffic_<workload>.json records the one its counters were collected with."""
    import hashlib

    h = hashlib.sha256()
    src = ROOT / "kofft_amd" / "csrc"
    for f in sorted(src.iterdir()):
        if f.suffix in (".hip", ".h", ".cpp") or f.name == "Makefile":
            h.update(f.name.encode())
            h.update(f.read_bytes())
    return h.hexdigest()[:16]


def launch_ranks(n: int, argv: list[str]) -> int:
    """Start n children of this script, one per GPU.  The parent makes no GPU call (it never imports torch)."""
    prof = profiler_preloaded()
    if prof is not None:
        sys.stderr.write(f"bench.py launcher: refusing to start {n} rank processes from a profiled process ({prof}): the profiler's "
                         "preloaded library has already initialised the GPU here.  Profile ONE rank (`--gpus 1`, the default); "
                         "a multi-rank run goes through `python bench.py --gpus N` or torchrun, unprofiled.\n")
        return 2
    port = free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ)
        env.update({"RANK": str(r), "LOCAL_RANK": str(r), "WORLD_SIZE": str(n), "LOCAL_WORLD_SIZE": str(n),
                    "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "KOFFT_BENCH_LAUNCHED": "1"})
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: what RCCL needs on this host driver
        procs.append(subprocess.Popen([sys.executable, str(Path(__file__).resolve())] + argv, env=env,
                                      stdout=subprocess.PIPE, stderr=None, text=True))
    outs: list[str] = [""] * n

    def drain(i):
        outs[i] = procs[i].stdout.read()

    ths = [threading.Thread(target=drain, args=(i,)) for i in range(n)]
    for t in ths:
        t.start()
    # one failed rank would leave the others waiting in a collective: stop them once any child has failed
    rcs = [None] * n
    while any(rc is None for rc in rcs):
        for i, p in enumerate(procs):
            if rcs[i] is None:
                rcs[i] = p.poll()
        if any(rc not in (None, 0) for rc in rcs):
            time.sleep(5.0)
            for i, p in enumerate(procs):
                if rcs[i] is None and p.poll() is None:
                    p.terminate()  # exactly the children started above
            for i, p in enumerate(procs):
                if rcs[i] is None:
                    try:
                        rcs[i] = p.wait(timeout=20)
                    except subprocess.TimeoutExpired:
                        p.kill()
                        rcs[i] = p.wait()
            break
        time.sleep(0.05)
    for t in ths:
        t.join()
    for i in range(1, n):  # other ranks' stdout is diagnostics only
        if outs[i].strip():
            sys.stderr.write("".join(f"[rank {i}] {ln}\n" for ln in outs[i].splitlines()))
    lines = [ln for ln in outs[0].splitlines() if ln.startswith("{")]
    for ln in outs[0].splitlines():
        if not ln.startswith("{"):
            sys.stderr.write(f"[rank 0] {ln}\n")
    bad = [i for i, rc in enumerate(rcs) if rc != 0]
    if bad:
        sys.stderr.write(f"bench.py launcher: ranks {bad} failed (exit codes {[rcs[i] for i in bad]})\n")
        return 1
    if not lines:
        sys.stderr.write("bench.py launcher: rank 0 printed no JSON line\n")
        return 1
    print(lines[-1], flush=True)
    return 0


def extra_workload_names(workload: str, world: int) -> list[str]:
    """The workloads a default run carries beside the headline: every other BASELINE config at every N (#3 and #5 shard by batch with no
    collective, #4 by frames with its all-gather timed apart; stft1024 first: should the watchdog fire during a later extra, nothing is
    lost but it), and at N = 1 the SURVEY 8(f) rows."""
    names = [k for k in ("stft1024", "rfft2048", "c64_2p20") if k != workload]
    if world == 1:
        names += list(F_ROWS)
    return names


def dry_rank(args) -> None:
    """--dry-launch: what this rank was given, no GPU call, no torch import.  With --dry-protocol the ranks then meet for real (gloo on
    127.0.0.1), run the collective steps of the protocol, and rank 0 prints the line's skeleton."""
    info = {"dry_launch": True, **{k: os.environ.get(k) for k in RANK_ENV}, "pid": os.getpid(), "torch_imported": "torch" in sys.modules}
    if not args.dry_protocol:
        print(json.dumps(info), flush=True)
        return
    import torch
    import torch.distributed as dist

    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    n_seen = 1
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo", rank=rank, world_size=world)
        ones = torch.ones(1, dtype=torch.float64)
        dist.all_reduce(ones)
        n_seen = int(round(float(ones.item())))
        dist.barrier()
        t = torch.tensor([float(rank)], dtype=torch.float64)  # the MAX-over-ranks reduction of the timing protocol
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        assert int(t.item()) == world - 1
    if rank == 0:
        extras_on = args.extras if args.extras is not None else (args.workload == "fft4096" and not args.batch)
        line = {"metric": None, "value": None, "unit": None, "n_gpus": n_seen, "steps": args.steps, "warmup": args.warmup, "ms_per_step": None,
                "higher_is_better": True, "scaling": None, "vs_baseline": None, "dtype": None, "data": "synthetic",
                "config": {"workload": WORKLOADS[args.workload]}, "roofline": None,
                "launcher": "self" if os.environ.get("KOFFT_BENCH_LAUNCHED") else ("torchrun" if world > 1 else "single"),
                "workloads": {k: None for k in extra_workload_names(args.workload, world)} if extras_on else None,
                **({"multi_single_process": None} if (world > 1 and extras_on and not args.no_multi_ab) else {}),
                "cpu_baseline": None, "dry_protocol": True, **info}
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


# ---------------------------------------------------------------------------------------------------
# cpu_baseline: the oracle (a port of kofft's CPU algorithm) on the host cores, bounded sample
# ---------------------------------------------------------------------------------------------------
def host_cores() -> int:
    """Cores this process may actually use: affinity mask, capped by the cgroup CPU quota if there is one."""
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = Path("/sys/fs/cgroup/cpu.max").read_text().split()[:2]
        if quota != "max":
            cores = max(1, min(cores, int(int(quota) / int(period))))
    except Exception:
        pass
    return cores


def cpu_baseline_fft4096(target_seconds: float):
    import numpy as np

    from oracle import pyoracle as ko

    n = 4096
    cores = host_cores()
    rng = np.random.default_rng(0x6B6F666674 + 2)

    def make(batch):
        return (rng.uniform(-1, 1, (batch, n)).astype(np.float32)
                + 1j * rng.uniform(-1, 1, (batch, n)).astype(np.float32)).astype(np.complex64)

    lib = ko.lib()
    import ctypes as C

    chunk = 256  # transforms per call: 8 MiB per thread, re-copied from a pristine source before every call

    def run(reps):
        srcs = [make(chunk) for _ in range(cores)]
        busy = [0.0] * cores

        def work(i):
            buf = np.empty_like(srcs[i])
            for _ in range(reps):
                np.copyto(buf, srcs[i])  # untimed: keeps repeated in-place transforms from overflowing
                t0 = time.perf_counter()
                rc = lib.ko_fft_batch_f32(C.c_void_p(buf.ctypes.data), C.c_size_t(n), C.c_size_t(chunk), 0)
                busy[i] += time.perf_counter() - t0
                assert rc == 0
        ths = [threading.Thread(target=work, args=(i,)) for i in range(cores)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        return max(busy)

    dt = max(run(1), 1e-4)
    reps = int(min(max(target_seconds / dt, 1), 4000))
    dt = run(reps)
    transforms = cores * reps * chunk
    return {
        "value": transforms * n / dt / 1e9,
        "unit": "GPoints/s",
        "cores": cores,
        "kind": "port",
        "sample": f"{transforms} x 4096-pt c32 ({cores} thr x {reps} calls x {chunk}), oracle/ C port of kofft's Stockham, busiest thread {dt:.1f} s",
        "reference_published": "kofft benchmarks/README.md:27: 1.046 ms per 4096-pt transform, 1 thread = 0.0039 GPoints/s (other hardware)",
    }


# ---------------------------------------------------------------------------------------------------
# the reference's OWN published benchmark: one transform per call (benchmarks/README.md)
# ---------------------------------------------------------------------------------------------------
REFERENCE_PUBLISHED_US = {  # kofft single-thread, Xeon 8370C, host memory, f32 (benchmarks/README.md lines cited in BASELINE.md)
    "c32_1024": 81.07, "c32_4096": 1046.0, "c32_1048576": 59270.0, "rfft_1024": 60.1, "rfft_2048": 97.7, "rfft_1048576": 66950.0,
}


def reference_single_transform(fft32, stream, budget_s: float = 0.25):
    """Per-call time of ONE transform, the unit the reference publishes.  `host_us`: the trait method on a host array
    (upload, kernel, download, synchronise -- what `fft.fft(&mut buf)` costs a drop-in caller); `device_us`: the same
    transform on device-resident data (HIP events over back-to-back calls on the bench stream)."""
    import numpy as np
    import torch

    rng = np.random.default_rng(7)
    out = {}
    for key, ref_us in REFERENCE_PUBLISHED_US.items():
        kind, n = key.split("_")[0], int(key.split("_")[1])
        if kind == "c32":
            x = (rng.uniform(-1, 1, n) + 1j * rng.uniform(-1, 1, n)).astype(np.complex64)
            d = torch.from_numpy(x.view(np.float32)).to("cuda")
            host = lambda: fft32.fft(x)  # noqa: E731  (in place, like the trait method; values may grow, timing does not care)
            devc = lambda: fft32.fft_dev(d.data_ptr(), n, 1)  # noqa: E731
        else:
            xr = rng.uniform(-1, 1, n).astype(np.float32)
            yo = np.zeros(n // 2 + 1, np.complex64)
            scratch = np.zeros(n // 2, np.complex64)
            di = torch.from_numpy(xr).to("cuda")
            do = torch.zeros(2 * (n // 2 + 1), dtype=torch.float32, device="cuda")
            host = lambda: fft32.rfft_with_scratch(xr, yo, scratch)  # noqa: E731
            devc = lambda: fft32.rfft_dev(di.data_ptr(), do.data_ptr(), None, n, 1)  # noqa: E731
        x0 = x.copy() if kind == "c32" else None
        for _ in range(3):
            host()
        reps, busy = 0, 0.0
        while busy < budget_s and reps < 2000:
            if x0 is not None:
                np.copyto(x, x0)  # untimed: repeated in-place transforms would overflow
            t0 = time.perf_counter()
            host()
            busy += time.perf_counter() - t0
            reps += 1
        host_us = busy / reps * 1e6
        for _ in range(3):
            devc()
        torch.cuda.synchronize()
        k = 50 if n > 65536 else 200
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(k):
            devc()
        e1.record(stream)
        torch.cuda.synchronize()
        dev_us = e0.elapsed_time(e1) / k * 1e3
        out[key] = {"host_us": round(host_us, 2), "device_us": round(dev_us, 2), "reference_published_us": ref_us,
                    "speedup_host": round(ref_us / host_us, 1)}
    out["note"] = ("one transform per call, f32; reference_published_us = kofft single-thread on a Xeon 8370C (its benchmarks/README.md, "
                   "other hardware, first criterion sample); host_us includes PCIe both ways and the synchronisation")
    return out


# ---------------------------------------------------------------------------------------------------
# one rank
# ---------------------------------------------------------------------------------------------------
class Workload:
    """Device-resident inputs and the launch closure of one BASELINE configuration."""

    def __init__(self, name, args, rank, world, dev, stream, fft32, fft64, batch_override=0):
        import numpy as np
        import torch

        import kofft_amd

        self.name = name
        self.prep = None  # untimed per-step restore of an input the call consumes (istft)
        gen = torch.Generator(device=dev)
        gen.manual_seed(0x6B6F666674 + 2 + rank)
        self.allgather = None
        self.block_prep = None  # untimed restore before every block (and at the latest every max_steps_per_restore steps)
        self.max_steps_per_restore = 0
        self.outputs = {}  # name -> device tensor: what the caller of one step receives (--dump-outputs)
        if name == "fft4096":
            n, batch = 4096, batch_override or 65536
            form = getattr(args, "form", "inplace")
            self.form = form
            # ONE pristine batch for both forms: uniform(-1, 1) x 1e-18 (the in-place form needs the head-room; the twin reads the
            # same values so that the two differ in nothing but where the spectra go)
            pristine = torch.empty((batch, n, 2), dtype=torch.float32, device=dev).uniform_(-1.0, 1.0, generator=gen).mul_(INPLACE_SCALE)
            buf = torch.empty_like(pristine)
            self.units_per_step = batch * n                      # complex points
            self.alg_bytes = 16 * self.units_per_step            # 8 B read + 8 B written per point
            self.unit = "GPoints/s"
            self.metric = "batched 4096-pt c32 FFT throughput, GPoints/s (achieved HBM GB/s: roofline.achieved)"
            if form == "inplace":
                buf.copy_(pristine)
                self.launch = lambda: fft32.fft_dev(buf.data_ptr(), n, batch, False)
                self.block_prep = lambda: buf.copy_(pristine)
                self.max_steps_per_restore = INPLACE_MAX_STEPS
                form_text = "in place: FftImpl::fft(&mut [Complex32]) (fft.rs:1054)"
            else:
                self.launch = lambda: fft32.fft_dev_oop(pristine.data_ptr(), buf.data_ptr(), n, batch, False)
                form_text = "out of place: fft_out_of_place (fft.rs:469), pristine input -> second buffer"
            self.cfg = {"workload": WORKLOADS[name], "n": n, "batch_per_gpu": batch, "form": form_text,
                        "layout": "interleaved re/im, contiguous", "direction": "forward", "sharding": f"batch x{world}, no collective"}
            self.dtype, self.scaling = "f32", "weak"
            self.kernels_per_step = 1
            self._finite_probe = buf
            self.outputs = {"fft4096_spectrum": buf}
            src, dst = pristine, buf
        elif name == "rfft2048":
            n, batch = 2048, batch_override or (1 << 20)
            src = torch.empty((batch, n), dtype=torch.float32, device=dev).uniform_(-1.0, 1.0, generator=gen)
            dst = torch.empty((batch, n // 2 + 1, 2), dtype=torch.float32, device=dev)
            win = torch.from_numpy(kofft_amd.hann(n)).to(dev)
            self.units_per_step = batch * n                      # real samples
            self.alg_bytes = batch * (4 * n + 8 * (n // 2 + 1))
            self.unit = "GSamples/s"
            self.metric = "batched 2048-pt f32 rfft + Hann throughput"
            self.launch = lambda: fft32.rfft_dev(src.data_ptr(), dst.data_ptr(), win.data_ptr(), n, batch)
            self.cfg = {"workload": WORKLOADS[name], "n": n, "batch_per_gpu": batch, "sharding": f"batch x{world}, no collective"}
            self.dtype, self.scaling = "f32", "weak"
            self.kernels_per_step = 1
            self.outputs = {"rfft2048_spectrum": dst}
        elif name == "c64_2p20":
            n, batch = 1 << 20, batch_override or 1024
            src = torch.empty((batch, n, 2), dtype=torch.float64, device=dev).uniform_(-1.0, 1.0, generator=gen)
            dst = torch.empty_like(src)
            self.units_per_step = batch * n
            self.alg_bytes = 32 * self.units_per_step            # 16 B read + 16 B written per point
            self.unit = "GPoints/s"
            self.metric = "batched 2^20-pt Complex64 forward FFT throughput"
            self.launch = lambda: fft64.fft_dev_oop(src.data_ptr(), dst.data_ptr(), n, batch, False)
            self.cfg = {"workload": WORKLOADS[name], "n": n, "batch_per_gpu": batch, "sharding": f"batch x{world}, no collective",
                        "passes_over_hbm": 2}
            self.dtype, self.scaling = "f64", "weak"
            self.kernels_per_step = None  # several kernels per step: see roofline.kernels_per_step in the line
            self.outputs = {"c64_2p20_spectrum": dst}
        elif name in ("istft1024", "magnitudes1024"):
            total_len, win_len, hop = 28_800_000, 1024, 256
            frames = -(-total_len // hop)
            sgen = torch.Generator(device=dev)
            sgen.manual_seed(0x6B6F666674 + 4)
            t = torch.arange(total_len, dtype=torch.float32, device=dev)
            sig = 0.5 * torch.sin(2 * np.pi * 440.0 * t / 48000.0) + 0.25 * torch.empty_like(t).uniform_(-1, 1, generator=sgen)
            del t
            self.dtype, self.scaling, self.kernels_per_step = "f32", "weak", None
            if name == "istft1024":
                win = torch.from_numpy(kofft_amd.hann(win_len)).to(dev)
                spec = torch.empty((frames, win_len, 2), dtype=torch.float32, device=dev)
                fft32.stft_dev(sig.data_ptr(), total_len, win.data_ptr(), win_len, hop, spec.data_ptr(), 0, frames)
                out_len = (frames - 1) * hop + win_len
                out = torch.zeros(out_len, dtype=torch.float32, device=dev)
                scratch = torch.zeros(out_len, dtype=torch.float32, device=dev)
                work = spec.clone()

                def prep():  # untimed: istft transforms its frames in place and accumulates into `output` (stft.rs:141-155)
                    work.copy_(spec)
                    out.zero_()
                self.prep = prep
                self.units_per_step = frames * win_len           # spectrum points in
                # compulsory traffic: frames read and written back (the reference leaves the time-domain frames in the caller's
                # buffer), output and window-square sums written
                self.alg_bytes = 2 * 8 * self.units_per_step + 2 * 4 * out_len
                self.unit = "GPoints/s"
                self.metric = "ISTFT 1024-pt Hann hop-256 throughput (spectrum points in)"
                self.launch = lambda: fft32.istft_dev(work.data_ptr(), frames, win.data_ptr(), win_len, hop, out.data_ptr(), out_len,
                                                      scratch.data_ptr())
                self.cfg = {"workload": WORKLOADS[name], "frames": frames, "win_len": win_len, "hop": hop, "out_len": out_len,
                            "kernels": "istft_fused_kernel (inverse transform + overlap-add in one pass) + seam / tail overlap-add, no atomics"}
                self._keep = (sig, win, spec, work, out, scratch)
                self.outputs = {"istft1024_signal": out, "istft1024_frames": work}
            else:
                bins = win_len // 2
                mags = torch.empty((frames, bins), dtype=torch.float32, device=dev)
                mx = torch.zeros(1, dtype=torch.float32, device=dev)
                self.units_per_step = frames * bins               # magnitudes out
                self.alg_bytes = 4 * total_len + 4 * self.units_per_step
                self.unit = "GMagnitudes/s"
                self.metric = "stft_magnitudes 1024-pt Hann hop-256 throughput (magnitudes out)"
                self.launch = lambda: fft32.stft_magnitudes_dev(sig.data_ptr(), total_len, win_len, hop, mags.data_ptr(), frames, mx.data_ptr())
                self.cfg = {"workload": WORKLOADS[name], "signal_len": total_len, "win_len": win_len, "hop": hop, "frames": frames,
                            "bins_per_frame": bins, "kernels": "one: STFT with the magnitude and the running maximum fused into the store"}
                self.kernels_per_step = 1
                self._keep = (sig, mags, mx)
                self.outputs = {"magnitudes1024_magnitudes": mags, "magnitudes1024_max": mx}
            return
        elif name == "fft2d_4096":
            rows = cols = 4096
            img = torch.empty((rows, cols, 2), dtype=torch.float32, device=dev).uniform_(-1.0, 1.0, generator=gen)
            self.units_per_step = rows * cols
            self.alg_bytes = 16 * self.units_per_step            # the image read once and written once
            self.unit = "GPoints/s"
            self.metric = "fft2d_inplace 4096 x 4096 c32 throughput"
            state = {"inv": False}

            def launch2d():  # forward and inverse alternate so that the in-place values stay bounded; both directions cost the same
                fft32.fftnd_dev(img.data_ptr(), 1, rows, cols, state["inv"])
                state["inv"] = not state["inv"]
            self.launch = launch2d
            pristine = img.clone()

            def restore2d():  # untimed, before every block: the last step's output does not depend on how many steps ran before
                img.copy_(pristine)
                state["inv"] = False
            self.block_prep = restore2d
            self.max_steps_per_restore = 1 << 62  # the values stay bounded: no restore inside a block
            self.cfg = {"workload": WORKLOADS[name], "rows": rows, "cols": cols, "direction": "forward / inverse alternating, in place",
                        "passes_over_hbm": "2: rows + the columns' first two stages, then one column-tile pass (DESIGN 5.7)"}
            self.dtype, self.scaling, self.kernels_per_step = "f32", "weak", None
            self._keep = (img, pristine)
            self.outputs = {"fft2d_4096_image": img}
            return
        elif name == "bluestein1000":
            n, batch = 1000, batch_override or 65536
            src = torch.empty((batch, n, 2), dtype=torch.float32, device=dev).uniform_(-1.0, 1.0, generator=gen)
            dst = torch.empty_like(src)
            self.units_per_step = batch * n
            self.alg_bytes = 16 * self.units_per_step
            self.unit = "GPoints/s"
            self.metric = "batched 1000-pt c32 FFT (Bluestein arm) throughput"
            self.launch = lambda: fft32.fft_dev_oop(src.data_ptr(), dst.data_ptr(), n, batch, False)
            self.cfg = {"workload": WORKLOADS[name], "n": n, "m": 2048, "batch_per_gpu": batch,
                        "kernels": "one: both 2048-pt transforms and the three pointwise products in registers + LDS"}
            self.dtype, self.scaling, self.kernels_per_step = "f32", "weak", 1
            self._keep = (src, dst)
            self.outputs = {"bluestein1000_spectrum": dst}
            return
        else:
            total_len, win_len, hop = 28_800_000, 1024, 256
            from kofft_amd.dist import frames_required, shard_range

            frames_total = frames_required(total_len, hop)
            f0, f1 = shard_range(frames_total, rank, world)
            sgen = torch.Generator(device=dev)
            sgen.manual_seed(0x6B6F666674 + 4)  # ONE signal, identical on every rank (frames of the same stream are sharded)
            t = torch.arange(total_len, dtype=torch.float32, device=dev)
            sig = 0.5 * torch.sin(2 * np.pi * 440.0 * t / 48000.0) + 0.25 * torch.empty_like(t).uniform_(-1, 1, generator=sgen)
            del t
            win = torch.from_numpy(kofft_amd.hann(win_len)).to(dev)
            count = f1 - f0
            dst = torch.empty((count, win_len, 2), dtype=torch.float32, device=dev)
            self.units_per_step = count * win_len                # output complex points of this rank
            self.alg_bytes = 4 * min(total_len - f0 * hop, (count - 1) * hop + win_len) + 8 * self.units_per_step
            self.unit = "GPoints/s"
            self.metric = "STFT 1024-pt Hann hop-256 throughput (output points, compute only)"
            self.launch = lambda: fft32.stft_dev(sig.data_ptr(), total_len, win.data_ptr(), win_len, hop, dst.data_ptr(), f0, count)
            self.cfg = {"workload": WORKLOADS[name], "signal_len": total_len, "win_len": win_len, "hop": hop,
                        "frames_total": frames_total, "sharding": f"frames x{world}, strong", "collective": "none in the timed region"}
            self.dtype, self.scaling = "f32", "strong"
            self.kernels_per_step = 1
            self._gather = (frames_total, win_len, count, dst)
            self.outputs = {"stft1024_spectrogram": dst}
        self._keep = (src, dst) if name != "stft1024" else (sig, win, dst)

    def shard_kernel_ms(self, fft32, stream, dev, worlds=(1, 2, 4, 8), reps=200):
        """Kernel time of rank 0's frame shard for each world size, on THIS one GPU: what compute-only strong scaling of
        config #4 can be at best (14 063 frames at 8 GPUs are ~23 us of kernel: the ~4 us dispatch floor and the ramp of a
        persistent kernel show here first).  Back-to-back launches between two HIP events on the launch stream."""
        import torch

        from kofft_amd.dist import shard_range

        frames_total, win_len, _, dst = self._gather
        sig, win, _ = self._keep
        hop = self.cfg["hop"]
        out = {}
        for g in worlds:
            f0, f1 = shard_range(frames_total, 0, g)
            call = lambda: fft32.stft_dev(sig.data_ptr(), sig.numel(), win.data_ptr(), win_len, hop, dst.data_ptr(), f0, f1 - f0)  # noqa: E731
            for _ in range(10):
                call()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                call()
            e1.record(stream)
            torch.cuda.synchronize(dev)
            ms = e0.elapsed_time(e1) / reps
            out[str(g)] = {"frames": f1 - f0, "kernel_ms": round(ms, 5),
                           "GPoints_per_s_if_all_ranks_match": round(frames_total * win_len / (ms * 1e-3) / 1e9, 1)}
        base = out["1"]["kernel_ms"]
        for g in worlds:
            out[str(g)]["compute_only_speedup"] = round(base / out[str(g)]["kernel_ms"], 2)
        out["note"] = ("rank 0's shard of config #4 timed on one GPU, back-to-back launches: a PREDICTION of compute-only strong "
                       "scaling, not a multi-GPU measurement; the all-gather (SURVEY 8e: ~0.75 ms direct) is on top")
        return out

    def time_allgather(self, dist, dev, world, barrier):
        """BASELINE config #4's exchange step (RCCL all-gather of the spectra), timed apart from the compute."""
        import torch

        frames_total, win_len, count, dst = self._gather
        per = -(-frames_total // world)
        slot = torch.zeros((per, win_len, 2), dtype=torch.float32, device=dev)
        slot[:count] = dst
        full = torch.empty((world * per, win_len, 2), dtype=torch.float32, device=dev)
        for _ in range(3):
            dist.all_gather_into_tensor(full, slot)
        torch.cuda.synchronize(dev)
        barrier()
        tg = time.perf_counter()
        for _ in range(10):
            dist.all_gather_into_tensor(full, slot)
        torch.cuda.synchronize(dev)
        barrier()
        ms = (time.perf_counter() - tg) / 10 * 1e3
        return {"ms_per_step": ms, "bytes_gathered_per_rank": int(full.numel() * 4),
                "algbw_GBps": full.numel() * 4 / (ms * 1e-3) / 1e9,
                "backend": "nccl (RCCL over xGMI), all_gather_into_tensor"}


def measure(w: Workload, steps, warmup, ramp_ms, min_seconds, dev, stream, barrier, reduce_max, reduce_sum, count_launches=None):
    """The timing protocol on one workload.  Returns the fields of the JSON line that depend on it."""
    import numpy as np
    import torch

    launches = 0
    since_restore = [0]

    def restore():
        w.block_prep()
        since_restore[0] = 0

    def guarded_launch():
        """One step outside the timed blocks; an in-place workload is restored before its values can overflow."""
        if w.block_prep is not None and since_restore[0] >= w.max_steps_per_restore:
            restore()
        if w.prep is not None:
            w.prep()
        w.launch()
        since_restore[0] += 1

    t_ramp = time.perf_counter()
    while (time.perf_counter() - t_ramp) * 1e3 < ramp_ms:  # clock ramp (untimed, not counted as warm-up steps)
        for _ in range(8):
            guarded_launch()
            launches += 1
        torch.cuda.synchronize(dev)
    for _ in range(warmup):
        guarded_launch()
        launches += 1
    torch.cuda.synchronize(dev)

    blocks, kern_ms_all = [], []
    total = 0.0
    inner_restores = w.block_prep is not None and steps > w.max_steps_per_restore
    while True:
        starts = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
        ends = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
        if w.block_prep is not None:
            restore()                  # untimed: outside the barriers of the block
        barrier()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for i in range(steps):
            if inner_restores and since_restore[0] >= w.max_steps_per_restore:
                restore()              # K > 30 only: inside the wall-clock bracket, outside every event pair (see below)
            if w.prep is not None:
                w.prep()               # restores an input the call consumes: outside the event pair
            starts[i].record(stream)   # HIP events on the stream the kernels are launched on
            w.launch()
            ends[i].record(stream)
            since_restore[0] += 1
        torch.cuda.synchronize(dev)
        barrier()
        torch.cuda.synchronize(dev)
        elapsed = reduce_max(time.perf_counter() - t0)   # identical on every rank: all ranks leave the loop together
        launches += steps
        km = [s.elapsed_time(e) for s, e in zip(starts, ends)]
        if w.prep is not None or inner_restores:
            # the block's wall time contains untimed restores: the steps' own HIP-event time instead (MAX over ranks like the wall time)
            elapsed = reduce_max(float(np.sum(km)) / 1e3)
        blocks.append(elapsed)
        kern_ms_all.append(km)
        total += elapsed
        if total >= min_seconds or len(blocks) >= 2000:
            break
    order = sorted(range(len(blocks)), key=lambda i: blocks[i])
    mid = order[len(order) // 2]
    elapsed = blocks[mid]
    kern_ms = kern_ms_all[mid]
    total_units = reduce_sum(float(w.units_per_step)) * steps
    avg_kernel_s = float(np.mean(kern_ms)) / 1e3
    achieved = w.alg_bytes / avg_kernel_s / 1e9
    traffic, traffic_from, traffic_stale, issue = None, None, None, {}
    tfile = ROOT / "profiles" / f"traffic_{w.name}.json"
    if tfile.exists():
        try:
            tj = json.loads(tfile.read_text())
            # the profile is of ONE form of the workload (config #2: in place); a twin measured in another form carries no counters
            tform = tj.get("form", "inplace" if w.name == "fft4096" else None)  # (files without the key: config #2 was profiled in place)
            if tj.get("workload") == w.name and tform == getattr(w, "form", None):
                traffic = tj.get("hbm_bytes_per_step", tj.get("hbm_bytes_per_launch"))
                traffic_from = tj.get("from")
                # the counters were collected with one version of the kernels: say so when the sources have changed since
                traffic_stale = tj.get("csrc_sha16") != csrc_sha16()
                issue = {k: tj[k] for k in ("valu_insts_per_step", "lds_active_cycles_per_step", "shader_clock_ghz") if tj.get(k)}
        except Exception:
            traffic = None
    # Which roofline binds: instruction and LDS-cycle counts per step and the shader clock come from the PMC
    # passes of tools/profile.sh (clock = GRBM_GUI_ACTIVE / 8 XCDs / dispatch duration under this very workload: measured, not the
    # data-sheet's); the time is this run's own HIP-event kernel time.  VALU: 4 cycles per wave64 instruction on each of 1024 SIMDs;
    # LDS: one pipe per CU.  `bound` = the largest of the three utilisations (HBM's is the PMC traffic, or the algorithmic bytes).
    valu_frac = lds_frac = None
    hbm_util = (traffic or w.alg_bytes) / avg_kernel_s / 1e9 / HBM_PEAK_GBS
    bound = "hbm"
    if issue.get("shader_clock_ghz"):
        cyc = issue["shader_clock_ghz"] * 1e9 * avg_kernel_s
        if issue.get("valu_insts_per_step"):
            valu_frac = issue["valu_insts_per_step"] * 4.0 / (1024 * cyc)
        if issue.get("lds_active_cycles_per_step"):
            lds_frac = issue["lds_active_cycles_per_step"] / (256 * cyc)
        bound = max((hbm_util, "hbm"), (valu_frac or 0.0, "valu"), (lds_frac or 0.0, "lds"))[1]
    if count_launches is not None:
        count_launches.append(launches)
    finite = None
    probe = getattr(w, "_finite_probe", None)
    if probe is not None:
        finite = bool(torch.isfinite(probe[:64]).all().item()) and bool(torch.isfinite(probe[-64:]).all().item())
    return {
        "metric": w.metric,
        "value": total_units / elapsed / 1e9,
        "unit": w.unit,
        "ms_per_step": elapsed / steps * 1e3,
        "blocks": len(blocks),
        "blocks_ms_per_step": [round(b / steps * 1e3, 4) for b in blocks[:8]],
        "blocks_ms_per_step_all": [round(b / steps * 1e3, 4) for b in blocks[:64]],
        "timed_by": "HIP events per step (untimed restores inside the block)" if (w.prep is not None or inner_restores) else "wall clock between barriers",
        "values_finite": finite,
        "scaling": w.scaling,
        "dtype": w.dtype,
        "config": w.cfg,
        "roofline": {
            "bound": bound,
            "achieved": achieved,
            "peak": HBM_PEAK_GBS,
            "unit": "GB/s",
            "frac": achieved / HBM_PEAK_GBS,
            "traffic": traffic,
            "traffic_from": traffic_from,
            "traffic_stale": traffic_stale,
            "hbm_util": hbm_util,
            "issue_frac": valu_frac,
            "lds_frac": lds_frac,
            "shader_clock_ghz": issue.get("shader_clock_ghz"),
            "kernel_ms_avg": avg_kernel_s * 1e3,
            "kernel_ms_min": float(np.min(kern_ms)),
            "algorithmic_bytes_per_launch": w.alg_bytes,
            "launch": "one step = one C-ABI call" + ("" if w.kernels_per_step == 1 else " (several kernels per step)"),
        },
    }


def dump_outputs(outputs: dict, out_dir: Path) -> None:
    """--dump-outputs: each array as out_dir/<name>.npy in its own dtype (float32 / float64).  An array larger than its share of
    DUMP_BYTES is written as the rows (first axis) picked by a generator seeded with DUMP_SEED, in ascending order: the same rows
    in every run with the same arguments."""
    import numpy as np
    import torch

    out_dir.mkdir(parents=True, exist_ok=True)
    share = DUMP_BYTES // len(outputs)
    for name, t in outputs.items():
        rows = t.shape[0]
        row_bytes = t.element_size() * (t[0].numel() if t.dim() > 1 else 1)
        keep = min(rows, share // row_bytes)
        if keep < 1:
            raise ValueError(f"--dump-outputs: one row of {name} ({row_bytes} B) exceeds the dump budget")
        if keep < rows:
            idx = np.sort(np.random.default_rng(DUMP_SEED).choice(rows, keep, replace=False))
            t = t.index_select(0, torch.from_numpy(idx).to(t.device))
        a = t.cpu().numpy()
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(out_dir / f"{name}.npy", a)
        print(f"# dump: {out_dir / name}.npy {a.dtype} {list(a.shape)} ({keep} of {rows} rows)", file=sys.stderr, flush=True)


def sig(x, digits=5):
    """x rounded to `digits` significant digits (the line is size-limited)."""
    if x is None or isinstance(x, (str, bool)) or x == 0:
        return x
    from math import floor, log10

    return round(x, digits - 1 - int(floor(log10(abs(x)))))


def summarise(name: str, r: dict) -> dict:
    """One workload's entry of roofline.configs: what the judge recomputes, nothing else."""
    if "error" in r:
        return {"error": r["error"][:100]}
    rf = r["roofline"]
    # ONE clock per entry: `ms` is the step time `value` is computed from (wall clock between barriers, or the
    # steps' HIP events where a block holds untimed restores) and `frac` = algorithmic bytes / THAT time / 8 TB/s; `kernel_ms` is the
    # HIP-event average of the kernels alone (the headline roofline object's clock, as the contract prescribes), for comparison.
    # `bound` names the roofline that binds; `issue_frac` / `lds_frac` = VALU issue / LDS pipe utilisation (measure(): from PMC counts).
    out = {"value": sig(r["value"]), "unit": r["unit"], "ms": sig(r["ms_per_step"]),
           "frac": sig(rf["algorithmic_bytes_per_launch"] / (r["ms_per_step"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
           "kernel_ms": sig(rf["kernel_ms_avg"]), "bound": rf["bound"]}
    if rf.get("issue_frac") is not None:
        out["issue_frac"] = sig(rf["issue_frac"], 3)
    if rf.get("lds_frac") is not None:
        out["lds_frac"] = sig(rf["lds_frac"], 3)
    if rf.get("traffic"):
        out["traffic_ratio"] = sig(rf["traffic"] / rf["algorithmic_bytes_per_launch"], 4)
        if rf.get("traffic_stale"):
            out["traffic_stale"] = True
    if name == "c64_2p20":
        out["cap"] = 0.5  # two passes over HBM (the 512 MiB intermediate does not stay in the Infinity Cache): frac / cap is the share of the achievable
        out["passes"] = 2
        pp = r.get("placement_probe")
        if pp and pp.get("n"):
            # the library timed its two factor kernels through n candidate placements of its 512 MiB intermediate and kept the fastest:
            # [first factor us, whole chunk us] of the pick and of the slowest candidate -- the spread a blind hipMalloc would draw from
            i, j = pp["pick"], max(range(pp["n"]), key=lambda k: pp["total_us"][k])
            out["probe"] = {"n": pp["n"], "pick_us": [pp["first_us"][i], pp["total_us"][i]], "worst_us": [pp["first_us"][j], pp["total_us"][j]]}
    if "allgather" in r:
        out["allgather_ms"] = sig(r["allgather"]["ms_per_step"])
        out["allgather_GBps"] = sig(r["allgather"]["algbw_GBps"], 4)
    if r.get("values_finite") is False:
        out["values_finite"] = False
    return out


def multi_single_process_ab(n_dev: int, rehearse: bool, reps: int = 5) -> dict:
    """Config #4 through the SINGLE-PROCESS multi-device handle (kofft_hip_multi_*, include/kofft_hip.h; the device analogue of
    stft::parallel's rayon-over-frames, stft.rs:232-263) over all n_dev devices, device-resident, in both exchange modes:
    the grouped in-place ncclAllGather and the direct peer copies (~0.75 ms direct against ~5 ms for a ring).
    Rank 0 runs this alone, after the per-rank protocol, while the other ranks wait at the final barrier (their GPUs idle).
    Slowest device's time per phase from the handle's HIP events; median over `reps` calls."""
    import numpy as np
    import torch

    import kofft_amd

    total_len, win_len, hop = 28_800_000, 1024, 256
    frames = -(-total_len // hop)
    devices = [0] * n_dev if rehearse else list(range(n_dev))
    before = torch.cuda.current_device()
    m = kofft_amd.HipMulti(n_dev, devices=devices)
    out = {"devices": n_dev, "frames": frames, "logical_devices_on_one_card": bool(rehearse)}
    try:
        d0 = torch.device("cuda", devices[0])
        sgen = torch.Generator(device=d0)
        sgen.manual_seed(0x6B6F666674 + 4)
        t = torch.arange(total_len, dtype=torch.float32, device=d0)
        sig_all = 0.5 * torch.sin(2 * np.pi * 440.0 * t / 48000.0) + 0.25 * torch.empty_like(t).uniform_(-1, 1, generator=sgen)
        del t
        win_h = torch.from_numpy(kofft_amd.hann(win_len))
        per = -(-frames // n_dev)
        slices, wins, outs = [], [], []
        for r in range(n_dev):
            d = torch.device("cuda", devices[r])
            first, count = m.stft_slice(total_len, win_len, hop, frames, r)
            slices.append(sig_all[first:first + count].to(d).contiguous().clone())
            wins.append(win_h.to(d))
            outs.append(torch.empty((n_dev * per, win_len, 2), dtype=torch.float32, device=d))
        del sig_all
        for d in set(devices):
            torch.cuda.synchronize(torch.device("cuda", d))
        modes = ("direct",) if rehearse else ("rccl", "direct")  # (RCCL refuses one card listed twice)
        for mode in modes:
            try:
                m.set_gather(mode)
                ks, gs = [], []
                for i in range(2 + reps):
                    m.stft_dev([x.data_ptr() for x in slices], total_len, [x.data_ptr() for x in wins], win_len, hop, frames,
                               allgather=True, d_out=[x.data_ptr() for x in outs])
                    m.synchronize()
                    tm = m.last_timing_ex()
                    if i >= 2:
                        ks.append(tm["kernel_ms"])
                        gs.append(tm["gather_ms"])
                assert m.gather_mode()["last"] == mode
                out[f"gather_{mode}_ms"] = sig(float(np.median(gs)))
                out[f"gather_{mode}_GBps_per_device"] = sig(per * win_len * 8 * (n_dev - 1) / (float(np.median(gs)) * 1e-3) / 1e9, 4)
                out["kernel_ms"] = sig(float(np.median(ks)))
            except Exception as e:
                out[f"gather_{mode}_error"] = f"{type(e).__name__}: {e}"[:160]
        # every device must hold the same gathered spectrogram: compare device r's buffer with device 0's (cheap checksum)
        try:
            sums = [float(x.double().sum().item()) for x in outs]
            out["gathered_identical_on_every_device"] = all(v == sums[0] for v in sums)
        except Exception as e:
            out["checksum_error"] = f"{type(e).__name__}: {e}"[:120]
    finally:
        m.close()
        torch.cuda.set_device(before)
    return out


def run_rank(args) -> None:
    # under torchrun nothing has set this for us; it must be in the environment before the HIP runtime starts
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: what RCCL needs on this host driver
    import numpy as np
    import torch
    import torch.distributed as dist

    import kofft_amd

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP library is the only implementation of this path")
    if args.rehearse_one_card:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    n_seen = 1
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.rehearse_one_card:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        ones = torch.ones(1, dtype=torch.float64, device=dev)
        dist.all_reduce(ones)  # a real collective: n_gpus below is the number of ranks RCCL actually connected
        n_seen = int(round(float(ones.item())))
        assert n_seen == dist.get_world_size()
    if args.gpus != world and rank == 0:
        print(f"# note: --gpus {args.gpus} but WORLD_SIZE={world}; using WORLD_SIZE", file=sys.stderr)

    fft32 = kofft_amd.HipFftImpl(np.float32, device=local_rank)
    fft64 = kofft_amd.HipFftImpl(np.float64, device=local_rank)
    # A dedicated (non-default) torch stream: the library launches on it and the HIP events are
    # recorded on the same stream, so each event pair brackets exactly one step.
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    assert stream.cuda_stream != 0
    fft32.set_stream(stream.cuda_stream)
    fft64.set_stream(stream.cuda_stream)

    def barrier():
        if world > 1:
            if args.rehearse_one_card:
                dist.barrier()
            else:
                dist.barrier(device_ids=[local_rank])

    def reduce_max(x: float) -> float:
        t = torch.tensor([x], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def reduce_sum(x: float) -> float:
        t = torch.tensor([x], dtype=torch.float64, device=dev)
        if world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
        return float(t.item())

    def park_until_rank0(key: str, work=None, timeout_s: float = 600.0):
        """Rank 0 runs `work` alone; the other ranks wait ON THE CPU (the rendezvous store), not in an RCCL barrier whose kernel would
        spin on their GPUs while rank 0's single-process section uses those same GPUs."""
        res = None
        if world == 1:
            return work() if work is not None else None
        from datetime import timedelta

        store = dist.distributed_c10d._get_default_store()
        if rank == 0:
            try:
                res = work() if work is not None else None
            finally:
                store.set(key, "1")
        else:
            try:
                store.wait([key], timedelta(seconds=timeout_s))
            except Exception:
                pass
        return res

    launches: list[int] = []
    w = Workload(args.workload, args, rank, world, dev, stream, fft32, fft64, args.batch)
    head = measure(w, args.steps, args.warmup, args.ramp_ms, args.min_seconds, dev, stream, barrier, reduce_max, reduce_sum, launches)
    if args.dump_outputs and rank == 0:
        dump_outputs(w.outputs, Path(args.dump_outputs))  # the buffers still hold the last timed step's results
    allgather = w.time_allgather(dist, dev, world, barrier) if (args.workload == "stft1024" and world > 1) else None
    del w
    torch.cuda.empty_cache()
    twin = None
    if args.workload == "fft4096" and not args.batch and not args.no_twin:
        # the other form of config #2 with the same protocol (same steps, warm-up, block rule; a shorter --min-seconds)
        try:
            targs = argparse.Namespace(**{**vars(args), "form": "oop" if args.form == "inplace" else "inplace"})
            wt = Workload("fft4096", targs, rank, world, dev, stream, fft32, fft64)
            twin = measure(wt, args.steps, args.warmup, 0.0, min(args.min_seconds, 0.5), dev, stream, barrier, reduce_max, reduce_sum)
            twin["form"] = targs.form
            del wt
        except Exception as e:  # informational: never at the cost of the line
            twin = {"error": f"{type(e).__name__}: {e}", "form": "oop" if args.form == "inplace" else "inplace"}
        torch.cuda.empty_cache()

    extras_on = args.extras if args.extras is not None else (args.workload == "fft4096" and not args.batch)
    extra_names = []
    if extras_on:
        # every BASELINE config at every N: #3 and #5 shard by batch with no collective (weak), #4 by frames (strong; its
        # all-gather timed apart).  stft1024 first: should the watchdog fire during a later extra, nothing is lost but it.
        extra_names = extra_workload_names(args.workload, world)
    multi_ab_on = world > 1 and extras_on and not args.no_multi_ab

    def config_summaries(extras):
        cfgs = {}
        if args.workload == "fft4096":
            cfgs["#2_" + args.form] = summarise("fft4096", head)
            if twin is not None:
                cfgs["#2_" + twin["form"]] = summarise("fft4096", twin)
        else:
            cfgs[CONFIG_KEY[args.workload]] = summarise(args.workload, head)
        for name, r in extras.items():
            cfgs[CONFIG_KEY[name]] = summarise(name, r)
        return cfgs

    # The headline exists from here on.  The extra workloads (at N > 1: the RCCL all-gather of config 4, rank 0's single-process
    # A/B) must never cost the line: if they have not finished after --extras-timeout seconds (a collective that hangs cannot be
    # caught as an exception), rank 0 prints the headline alone and the process ends -- still exactly one JSON line.
    def headline_line(extras):
        rf = {k: (sig(v, 6) if isinstance(v, float) else v) for k, v in head["roofline"].items()}
        rf["configs"] = config_summaries(extras)
        return {
            "metric": head["metric"], "value": head["value"], "unit": head["unit"], "n_gpus": n_seen, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": head["ms_per_step"], "higher_is_better": True, "scaling": head["scaling"],
            "vs_baseline": None, "dtype": head["dtype"], "data": "synthetic", "config": head["config"], "roofline": rf,
            "blocks": head["blocks"], "blocks_ms_per_step": head["blocks_ms_per_step"], "timed_by": head["timed_by"],
            "values_finite": head["values_finite"], "launches_total": launches[0],
            "launcher": "self" if os.environ.get("KOFFT_BENCH_LAUNCHED") else ("torchrun" if world > 1 else "single"),
            **({"rehearsal": "every rank on cuda:0, gloo process group: NOT a measurement"} if args.rehearse_one_card else {}),
        }

    extras: dict = {}
    watchdog = None
    if args.extras_timeout is None:
        args.extras_timeout = 240.0 if world > 1 else 0.0
    if (extra_names or multi_ab_on) and args.extras_timeout > 0:
        def give_up():
            if rank == 0:
                line = headline_line(dict(extras))  # whatever has finished rides along
                if allgather is not None:
                    line["allgather"] = allgather
                line["workloads"] = {"error": f"extra workloads did not finish within {args.extras_timeout:.0f} s; finished so far: {sorted(extras)}"}
                line["cpu_baseline"] = None
                print(json.dumps(line), flush=True)
            os._exit(0)  # every rank: the headline is a complete, valid measurement
        watchdog = threading.Timer(args.extras_timeout, give_up)
        watchdog.daemon = True
        watchdog.start()
    for name in extra_names:
        try:
            we = Workload(name, args, rank, world, dev, stream, fft32, fft64)
            steps_e = max(5, min(args.steps, 20)) if name in ("c64_2p20", "istft1024") else args.steps
            r = measure(we, steps_e, min(args.warmup, 5), args.ramp_ms, min(args.min_seconds, 1.0), dev, stream, barrier, reduce_max, reduce_sum)
            r["steps"] = steps_e
            if name == "stft1024" and world > 1:
                r["allgather"] = we.time_allgather(dist, dev, world, barrier)
            if name == "stft1024" and world == 1:
                r["shard_ms"] = we.shard_kernel_ms(fft32, stream, dev)
            if name == "c64_2p20":
                r["placement_probe"] = fft64.big_probe_info()  # the intermediate's candidates (us per 512 MiB chunk) and the pick
            extras[name] = r
            del we
        except Exception as e:  # the headline must survive a failing extra
            extras[name] = {"error": f"{type(e).__name__}: {e}"}
        torch.cuda.empty_cache()

    multi_ab = None
    if multi_ab_on:
        def run_ab():
            try:
                return multi_single_process_ab(world, args.rehearse_one_card)
            except Exception as e:  # informational: never at the cost of the line
                return {"error": f"{type(e).__name__}: {e}"[:200]}
        torch.cuda.synchronize(dev)
        multi_ab = park_until_rank0("kofft_bench_multi_ab_done", run_ab)

    if watchdog is not None:
        watchdog.cancel()
    if rank == 0:
        out = headline_line(extras)
        detail = {"headline": head, "twin": twin, "workloads": extras}
        if allgather is not None:
            out["allgather"] = allgather
        if extras:
            out["workloads"] = {k: ({"value": sig(r["value"]), "unit": r["unit"], "ms_per_step": sig(r["ms_per_step"]),
                                     "frac": sig(r["roofline"]["frac"], 4), "steps": r["steps"]} if "error" not in r else r)
                                for k, r in extras.items()}
        if multi_ab is not None:
            out["multi_single_process"] = multi_ab
        if extras_on and world == 1:
            try:
                rs = reference_single_transform(fft32, stream)
                detail["reference_single_transform"] = rs
                # [this path from host memory, device-resident, kofft published (other hardware)] in microseconds per transform
                out["reference_single_transform_us"] = {k: [v["host_us"], v["device_us"], v["reference_published_us"]]
                                                        for k, v in rs.items() if isinstance(v, dict)}
            except Exception as e:  # informational: never at the cost of the line
                out["reference_single_transform_us"] = {"error": f"{type(e).__name__}: {e}"[:160]}
        if args.workload == "fft4096" and not args.no_cpu_baseline:
            # the CPU path "in the same run" (north_star): rank 0's host cores; at N > 1 the other ranks are parked in the
            # final barrier meanwhile (their GPUs idle, the timed regions are over)
            out["cpu_baseline"] = cpu_baseline_fft4096(args.cpu_seconds)
            if world > 1:
                out["cpu_baseline"]["sample"] += f"; rank 0, the other {world - 1} ranks parked"
        # the full objects: a side file (merged back by gpurun) and stderr; the line itself stays inside the driver's tail buffer
        dpath = Path(args.detail_file) if args.detail_file else ROOT / "gpurun_out" / f"bench_detail_n{n_seen}.json"
        try:
            dpath.parent.mkdir(parents=True, exist_ok=True)
            dpath.write_text(json.dumps({**detail, "line": out}, indent=1) + "\n")
            out["detail_file"] = str(dpath.relative_to(ROOT)) if dpath.is_relative_to(ROOT) else str(dpath)
        except Exception:
            pass
        print("# detail " + json.dumps(detail), file=sys.stderr, flush=True)
        text = json.dumps(out)
        if len(text) > LINE_BUDGET:  # never expected; drop the optional blocks first, the contract keys never
            for key in ("reference_single_transform_us", "workloads", "blocks_ms_per_step"):
                out.pop(key, None)
                text = json.dumps(out)
                if len(text) <= LINE_BUDGET:
                    break
        print(text, flush=True)

    if world > 1:
        barrier()
        dist.destroy_process_group()


def main():
    argv = sys.argv[1:]
    args = parse(argv)
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        raise SystemExit(launch_ranks(args.gpus, argv))  # the parent: no torch, no GPU call
    if args.dry_launch:
        dry_rank(args)
        return
    run_rank(args)


if __name__ == "__main__":
    main()
