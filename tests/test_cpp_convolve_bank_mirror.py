"""Builds and runs tests/cpp/test_convolve_bank_mirror.cpp: the C++ host mirror of the filter-bank convolution (include/kofft_hip.hpp:
convolve_bank_rows / set_convolve_bank_fused) against a direct sum in double, route against route, one real filter against
convolve_rows, the real part and the magnitude against the complex values and windows against the full result bit for bit, and the
mirror's length errors, linked to libkofft_hip.so."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "tests" / "cpp" / "test_convolve_bank_mirror"


def build():
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", str(ROOT / "tests/cpp/test_convolve_bank_mirror.cpp"), "-o", str(EXE),
           f"-L{ROOT / 'kofft_amd/lib'}", "-lkofft_hip", f"-Wl,-rpath,{ROOT / 'kofft_amd/lib'}", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)


def test_cpp_convolve_bank_mirror_compiles():
    """CPU: the header's bank methods and the driver translate and link against the C ABI (no GPU needed to build)."""
    build()
    assert EXE.exists()


@pytest.mark.gpu
def test_cpp_convolve_bank_mirror_runs():
    build()
    res = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 failed" in res.stdout
