"""Builds and runs tests/cpp/test_pfb_mirror.cpp: the C++ host mirror of the polyphase filter bank (include/kofft_hip.hpp:
pfb_analysis_rows / pfb_synthesis_rows / set_pfb_fused / pfb_taps / pfb_reconstruction) against vectors this test writes -- inputs and
the outputs of tests/pfb_oracle.py, compared bit for bit on both routes -- and the mirror's own errors, linked to libkofft_hip.so."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pfb_oracle as po

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "tests" / "cpp" / "test_pfb_mirror"
F = np.float32

# (M, T, D, rows, nx, lead, frames, bins): fused and composed lengths, a Bluestein one, both forms of bins, leads other than 0
CASES = [(64, 4, 64, 3, 700, 0, 13, 33), (1024, 2, 512, 2, 5000, 1536, 14, 513), (4096, 1, 2048, 1, 20000, 2048, 11, 4096),
         (2, 3, 1, 3, 9, 5, 16, 2), (240, 3, 100, 3, 1500, 620, 22, 121), (8192, 2, 8192, 1, 40000, 8192, 6, 4097)]


def build():
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", str(ROOT / "tests/cpp/test_pfb_mirror.cpp"), "-o", str(EXE),
           f"-L{ROOT / 'kofft_amd/lib'}", "-lkofft_hip", f"-Wl,-rpath,{ROOT / 'kofft_amd/lib'}", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)


def write_vectors(path):
    """u64 count; per case eight u64 (M, T, D, rows, nx, lead, frames, bins) and the f32 scale, then x and the taps as f32, the
    oracle's analysis as complex64 and the whole overlap-added synthesis of it (taps as the synthesis filter) as f32."""
    rng = np.random.default_rng(34400)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(CASES)))
        for m, taps, hop, rows, nx, lead, frames, bins in CASES:
            x = rng.uniform(-1, 1, (rows, nx)).astype(F)
            h = rng.uniform(0.1, 1, taps * m).astype(F)
            scale = F(0.5)
            Z = po.analysis_ref(x, h, m, hop, lead, frames, bins)
            y = po.synthesis_ref(Z, h, m, hop, scale)
            f.write(struct.pack("<8Q", m, taps, hop, rows, nx, lead, frames, bins) + scale.tobytes())
            f.write(x.tobytes() + h.tobytes() + Z.tobytes() + y.tobytes())


def test_cpp_pfb_mirror_compiles():
    """CPU: the header's methods and the driver translate and link against the C ABI (no GPU needed to build)."""
    build()
    assert EXE.exists()


@pytest.mark.gpu
def test_cpp_pfb_mirror_runs(oracle, tmp_path):
    build()
    vectors = tmp_path / "pfb_vectors.bin"
    write_vectors(vectors)
    res = subprocess.run([str(EXE), str(vectors)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 failed" in res.stdout and f"{len(CASES)} cases" in res.stdout
