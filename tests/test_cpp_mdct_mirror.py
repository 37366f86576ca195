"""Builds and runs tests/cpp/test_mdct_mirror.cpp: the C++ host mirror of the fast DCT-IV, the MDCT and the IMDCT (include/kofft_hip.hpp:
dct4_fast_rows / mdct_rows / imdct_rows / set_mdct_fused) against vectors this test writes -- inputs and the outputs of
tests/mdct_oracle.py, compared bit for bit on both routes -- and the mirror's own errors, linked to libkofft_hip.so."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import mdct_oracle as mo

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "tests" / "cpp" / "test_mdct_mirror"
F = np.float32

# (N, rows, nx, lead, frames): fused and composed lengths, a Bluestein one, leads other than N
CASES = [(64, 3, 300, 64, 6), (1024, 2, 3000, 1024, 4), (8192, 1, 20000, 1, 4), (2, 3, 9, 2, 6), (240, 3, 1000, 0, 5), (16384, 1, 40000, 16384, 4)]


def build():
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", str(ROOT / "tests/cpp/test_mdct_mirror.cpp"), "-o", str(EXE),
           f"-L{ROOT / 'kofft_amd/lib'}", "-lkofft_hip", f"-Wl,-rpath,{ROOT / 'kofft_amd/lib'}", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)


def write_vectors(path):
    """u64 count; per case five u64 (N, rows, nx, lead, frames) and the f32 scale, then as f32: x, the window, the oracle's DCT-IV of
    its own MDCT coefficients (frame by frame), those coefficients, and the whole overlap-added IMDCT of them."""
    rng = np.random.default_rng(32400)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(CASES)))
        for n, rows, nx, lead, frames in CASES:
            x = rng.uniform(-1, 1, (rows, nx)).astype(F)
            w = rng.uniform(0.1, 1, 2 * n).astype(F)
            scale = F(2.0 / n)
            X = mo.mdct_ref(x, w, lead, frames)
            d = mo.dct4_ref(X.reshape(rows * frames, n))
            y = mo.imdct_ref(X, w, scale)
            f.write(struct.pack("<5Q", n, rows, nx, lead, frames) + scale.tobytes())
            f.write(x.tobytes() + w.tobytes() + d.tobytes() + X.tobytes() + y.tobytes())


def test_cpp_mdct_mirror_compiles():
    """CPU: the header's methods and the driver translate and link against the C ABI (no GPU needed to build)."""
    build()
    assert EXE.exists()


@pytest.mark.gpu
def test_cpp_mdct_mirror_runs(oracle, tmp_path):
    build()
    vectors = tmp_path / "mdct_vectors.bin"
    write_vectors(vectors)
    res = subprocess.run([str(EXE), str(vectors)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 failed" in res.stdout and f"{len(CASES)} cases" in res.stdout
