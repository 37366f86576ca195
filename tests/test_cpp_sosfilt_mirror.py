"""Builds and runs tests/cpp/test_sosfilt_mirror.cpp: the C++ host mirror of the batched IIR filter (include/kofft_hip.hpp:
sosfilt_rows / set_sosfilt_tiled) against vectors this test writes -- inputs and the outputs and final states of
tests/sosfilt_oracle.py, compared bit for bit on both routes, out of place and in place -- and the mirror's own errors, linked to
libkofft_hip.so."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from sosfilt_oracle import cascade, sosfilt_ref

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "tests" / "cpp" / "test_sosfilt_mirror"
F = np.float32

# (rows, nx, sections, reverse, with an initial state)
CASES = [(1, 50, 1, 0, 0), (3, 69, 2, 0, 1), (65, 100, 3, 1, 1), (130, 37, 9, 0, 1), (67, 161, 17, 1, 1), (2, 1, 2, 1, 0), (300, 8, 1, 0, 1)]


def build():
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", str(ROOT / "tests/cpp/test_sosfilt_mirror.cpp"), "-o", str(EXE),
           f"-L{ROOT / 'kofft_amd/lib'}", "-lkofft_hip", f"-Wl,-rpath,{ROOT / 'kofft_amd/lib'}", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)


def write_vectors(path):
    """u64 count; per case five u64 (rows, nx, sections, reverse, with_zi), then x, sos, zi (zeros without one), the oracle's output and
    final state as f32."""
    rng = np.random.default_rng(30800)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(CASES)))
        for rows, nx, sections, reverse, with_zi in CASES:
            x = rng.uniform(-1, 1, (rows, nx)).astype(F)
            sos = cascade(sections)
            zi = rng.uniform(-1, 1, (rows, sections, 2)).astype(F) if with_zi else np.zeros((rows, sections, 2), F)
            y, zf = sosfilt_ref(sos, x, zi, bool(reverse))
            f.write(struct.pack("<5Q", rows, nx, sections, reverse, with_zi))
            f.write(x.tobytes() + sos.tobytes() + zi.tobytes() + y.tobytes() + zf.tobytes())


def test_cpp_sosfilt_mirror_compiles():
    """CPU: the header's sosfilt methods and the driver translate and link against the C ABI (no GPU needed to build)."""
    build()
    assert EXE.exists()


@pytest.mark.gpu
def test_cpp_sosfilt_mirror_runs(tmp_path):
    build()
    vectors = tmp_path / "sosfilt_vectors.bin"
    write_vectors(vectors)
    res = subprocess.run([str(EXE), str(vectors)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 failed" in res.stdout and f"{len(CASES)} cases" in res.stdout
