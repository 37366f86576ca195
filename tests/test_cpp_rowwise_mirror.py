"""Builds and runs tests/cpp/test_rowwise_mirror.cpp: the C++ host mirror's dct2, hilbert_analytic, real_cepstrum, dct_direct and
dst_direct (include/kofft_hip.hpp) against the C ABI and the C oracle's ko_direct_f32, linked to libkofft_hip.so and the oracle."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "tests" / "cpp" / "test_rowwise_mirror"


def build():
    from oracle import pyoracle

    pyoracle.build()
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", str(ROOT / "tests/cpp/test_rowwise_mirror.cpp"), "-o", str(EXE),
           f"-L{ROOT / 'kofft_amd/lib'}", "-lkofft_hip", f"-L{ROOT / 'oracle'}", "-lkofft_oracle",
           f"-Wl,-rpath,{ROOT / 'kofft_amd/lib'}", f"-Wl,-rpath,{ROOT / 'oracle'}", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)


def test_cpp_rowwise_mirror_compiles():
    """CPU: the header's row-wise methods and the driver translate and link against the C ABI and the oracle (no GPU needed)."""
    build()
    assert EXE.exists()


@pytest.mark.gpu
def test_cpp_rowwise_mirror_runs():
    build()
    res = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 failed" in res.stdout
