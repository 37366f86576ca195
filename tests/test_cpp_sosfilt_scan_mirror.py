"""Builds and runs tests/cpp/test_sosfilt_scan_mirror.cpp: the C++ host mirror of the IIR filter as a scan along time
(include/kofft_hip.hpp: sosfilt_scan_rows / sosfilt_scan_chunk) against vectors this test writes -- inputs and the outputs and final
states of tests/sosfilt_scan_oracle.py, compared bit for bit, out of place and in place -- and the mirror's own errors, linked to
libkofft_hip.so."""
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from sosfilt_oracle import cascade
from sosfilt_scan_oracle import sosfilt_scan_ref

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "tests" / "cpp" / "test_sosfilt_scan_mirror"
F = np.float32

# (rows, nx, sections, reverse, with an initial state, chunk)
CASES = [(1, 50, 1, 0, 0, 32), (3, 43 * 32 - 7, 2, 0, 1, 32), (5, 700, 3, 1, 1, 64), (2, 130 * 32 + 1, 9, 0, 1, 32), (67, 161, 17, 1, 1, 96),
         (2, 1, 2, 1, 0, 32), (3, 200, 4, 0, 1, 1024)]


def build():
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", str(ROOT / "tests/cpp/test_sosfilt_scan_mirror.cpp"), "-o", str(EXE),
           f"-L{ROOT / 'kofft_amd/lib'}", "-lkofft_hip", f"-Wl,-rpath,{ROOT / 'kofft_amd/lib'}", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)


def write_vectors(path):
    """u64 count; per case six u64 (rows, nx, sections, reverse, with_zi, chunk), then x, sos, zi (zeros without one), the oracle's output
    and final state as f32."""
    rng = np.random.default_rng(32300)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(CASES)))
        for rows, nx, sections, reverse, with_zi, chunk in CASES:
            x = rng.uniform(-1, 1, (rows, nx)).astype(F)
            sos = cascade(sections)
            zi = rng.uniform(-1, 1, (rows, sections, 2)).astype(F) if with_zi else np.zeros((rows, sections, 2), F)
            y, zf = sosfilt_scan_ref(sos, x, chunk, zi, bool(reverse))
            f.write(struct.pack("<6Q", rows, nx, sections, reverse, with_zi, chunk))
            f.write(x.tobytes() + sos.tobytes() + zi.tobytes() + y.tobytes() + zf.tobytes())


def test_cpp_sosfilt_scan_mirror_compiles():
    """CPU: the header's scan methods and the driver translate and link against the C ABI (no GPU needed to build)."""
    build()
    assert EXE.exists()


@pytest.mark.gpu
def test_cpp_sosfilt_scan_mirror_runs(tmp_path):
    build()
    vectors = tmp_path / "sosfilt_scan_vectors.bin"
    write_vectors(vectors)
    res = subprocess.run([str(EXE), str(vectors)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 failed" in res.stdout and f"{len(CASES)} cases" in res.stdout
