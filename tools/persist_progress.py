#!/usr/bin/env python3
"""How the workgroups of the 4096-point c32 streaming kernel progress relative to each other: one record per workgroup from a
diagnostic build (ONLY=k_complex_f32 tools/build_variant.sh stamps -DKOFFT_PERSIST_STAMPS; fft_persist.hip.h).  Lane 0 of every
workgroup's first wavefront stamps the kernel's entry, the landing of its first row's loads and the issue of its last row's stores
(s_memtime, and s_memrealtime -- the constant 100 MHz clock, the one that compares workgroups on different XCDs), counts its rows and
reads where it runs (HW_REG_HW_ID: CU bits 11:8, SH bit 12, SE bits 15:13; HW_REG_XCC_ID bits 3:0).

The full-size shape (65536 x 4096, forward) runs once out of place and once in place after a few warm-up launches; for each the tool
prints and writes: workgroups per CU, the distribution of start and finish times inside the kernel's own span (first start .. last
finish), the mean finish per XCD, rows per workgroup, and the share of wave-time missing at the start and at the end.  A diagnostic
build's run time is not the product's: read the shares.

usage (GPU box): KOFFT_HIP_LIB=kofft_amd/lib_stamps/libkofft_hip.so python3 tools/persist_progress.py [--claim-pct P] [--out profiles/FILE.txt]"""
import argparse
import ctypes as C
import os
import sys
from collections import Counter
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402

N, BATCH, WGS, WORDS = 4096, 65536, 4096, 16
REAL_US = 0.01  # s_memrealtime: 100 MHz


def quantiles(v):
    return [float(np.percentile(v, q)) for q in (0, 25, 50, 75, 95, 100)]


def report(tag, rec, kernel_ms, out):
    rec = rec[rec[:, 10] == 1]
    grid = int(rec[0, 9])
    t0, t1, t2, rows = rec[:, 3].astype(np.int64), rec[:, 4].astype(np.int64), rec[:, 5].astype(np.int64), rec[:, 6].astype(np.int64)
    hw, xcc = rec[:, 7].astype(np.int64), rec[:, 8].astype(np.int64) & 15
    cu, sh, se = (hw >> 8) & 15, (hw >> 12) & 1, (hw >> 13) & 7
    first, last = t0.min(), t2.max()
    span = float(last - first)
    out(f"== {tag}: grid {grid} workgroups, {len(rec)} records, rows {rows.sum()} (min {rows.min()} / mean {rows.mean():.1f} / max {rows.max()} per workgroup)")
    out(f"   span first start .. last finish {span * REAL_US:.1f} us (events around the launch: {kernel_ms * 1e3:.1f} us)")
    per_cu = Counter(zip(xcc.tolist(), se.tolist(), sh.tolist(), cu.tolist()))
    out(f"   CUs in use {len(per_cu)}; workgroups per CU: " + ", ".join(f"{k} on {v} CUs" for k, v in sorted(Counter(per_cu.values()).items())))
    out(f"   {'':22s}      min      q25   median      q75      p95      max")
    for name, v in (("start", t0 - first), ("first row landed", t1 - first), ("finish", t2 - first), ("resident", t2 - t0)):
        q = quantiles(v)
        out(f"   {name:22s} " + " ".join(f"{x * REAL_US:8.1f}" for x in q) + "   us")
        out(f"   {'  share of the span':22s} " + " ".join(f"{x / span:8.4f}" for x in q))
    out("   per XCD: workgroups, mean start, mean finish (us), mean rows")
    for x in sorted(set(xcc.tolist())):
        m = xcc == x
        out(f"     XCD {x}: {int(m.sum()):4d}  {(t0[m] - first).mean() * REAL_US:8.1f}  {(t2[m] - first).mean() * REAL_US:8.1f}  {rows[m].mean():8.1f}")
    miss_start = (t0 - first).mean() / span
    miss_end = (last - t2).mean() / span
    out(f"   wave-time missing at the start {miss_start:.4f}, at the end {miss_end:.4f} of the span; resident {1 - miss_start - miss_end:.4f}")
    ticks = (rec[:, 2].astype(np.int64) - rec[:, 0].astype(np.int64)) / np.maximum(t2 - t0, 1)
    out(f"   s_memtime ticks per 10 ns of s_memrealtime while resident: median {np.median(ticks):.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--claim-pct", type=int, default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--warm", type=int, default=5)
    args = ap.parse_args()
    import torch

    path = os.environ.get("KOFFT_HIP_LIB", "kofft_amd/lib_stamps/libkofft_hip.so")
    lib = C.CDLL(path)
    lib.kofft_hip_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    lib.kofft_hip_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.kofft_hip_fft_c32_dev_oop.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int]
    lib.kofft_hip_fft_c32_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int]
    lib.kofft_hip_exp_persist_stamps_f32.argtypes = [C.c_void_p, C.c_size_t]
    ctx = C.c_void_p()
    assert lib.kofft_hip_create(0, C.byref(ctx)) == 0
    if args.claim_pct is not None:
        lib.kofft_hip_set_persist_claim_pct.argtypes = [C.c_void_p, C.c_int]
        assert lib.kofft_hip_set_persist_claim_pct(ctx, args.claim_pct) == 0
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    assert lib.kofft_hip_set_stream(ctx, C.c_void_p(stream.cuda_stream)) == 0
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    pristine = torch.empty((BATCH, N, 2), dtype=torch.float32, device=dev).uniform_(-1.0, 1.0, generator=g).mul_(1e-18)
    src, dst = pristine.clone(), torch.empty_like(pristine)
    lines = []

    def out(s):
        print(s, flush=True)
        lines.append(s)

    out(f"library {path}, claim pct {'default' if args.claim_pct is None else args.claim_pct}")
    forms = (("out of place", lambda: lib.kofft_hip_fft_c32_dev_oop(ctx, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), N, BATCH, 0)),
             ("in place", lambda: lib.kofft_hip_fft_c32_dev(ctx, C.c_void_p(dst.data_ptr()), N, BATCH, 0)))
    for tag, call in forms:
        for _ in range(args.warm):
            dst.copy_(pristine)
            assert call() == 0
        dst.copy_(pristine)
        torch.cuda.synchronize(dev)
        assert lib.kofft_hip_exp_persist_stamps_clear_f32() == 0
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        assert call() == 0
        b.record(stream)
        torch.cuda.synchronize(dev)
        buf = np.zeros(WGS * WORDS, dtype=np.uint64)
        assert lib.kofft_hip_exp_persist_stamps_f32(buf.ctypes.data, buf.nbytes) == 0
        report(tag, buf.reshape(WGS, WORDS), a.elapsed_time(b), out)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
