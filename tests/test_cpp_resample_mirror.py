"""Builds and runs tests/cpp/test_resample_mirror.cpp: the C++ host mirror of the polyphase resampler (include/kofft_hip.hpp:
resample_rows / set_resample_tiled / resample_taps) against vectors this test writes -- inputs and the outputs of
tests/resample_oracle.py, compared bit for bit on both routes -- and the mirror's own errors, linked to libkofft_hip.so."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from resample_oracle import full_len, resample_ref

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "tests" / "cpp" / "test_resample_mirror"
F = np.float32

# (up, down, rows, nx, nh, t0, out_len or None for the full result from time 0)
CASES = [(1, 1, 2, 300, 5, 0, None), (3, 2, 3, 1500, 31, 0, None), (1, 3, 3, 3100, 61, 30, 1034), (160, 441, 2, 3000, 1765, 7, 1000),
         (441, 160, 1, 700, 1765, 0, None), (7, 2, 3, 40, 3, 0, None), (3, 2, 2, 700, 20001, 0, None)]


def build():
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", str(ROOT / "tests/cpp/test_resample_mirror.cpp"), "-o", str(EXE),
           f"-L{ROOT / 'kofft_amd/lib'}", "-lkofft_hip", f"-Wl,-rpath,{ROOT / 'kofft_amd/lib'}", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)


def write_vectors(path):
    """u64 count; per case seven u64 (up, down, rows, nx, nh, t0, out_len), then x, h and the oracle's output as f32."""
    rng = np.random.default_rng(28400)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(CASES)))
        for up, down, rows, nx, nh, t0, out_len in CASES:
            if out_len is None:
                out_len = full_len(nx, nh, up, down)
            x = rng.uniform(-1, 1, (rows, nx)).astype(F)
            h = rng.uniform(-1, 1, nh).astype(F)
            want = resample_ref(x, h, up, down, t0, out_len)
            f.write(struct.pack("<7Q", up, down, rows, nx, nh, t0, out_len))
            f.write(x.tobytes() + h.tobytes() + want.tobytes())


def test_cpp_resample_mirror_compiles():
    """CPU: the header's resample methods and the driver translate and link against the C ABI (no GPU needed to build)."""
    build()
    assert EXE.exists()


@pytest.mark.gpu
def test_cpp_resample_mirror_runs(tmp_path):
    build()
    vectors = tmp_path / "resample_vectors.bin"
    write_vectors(vectors)
    res = subprocess.run([str(EXE), str(vectors)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 failed" in res.stdout and f"{len(CASES)} cases" in res.stdout
