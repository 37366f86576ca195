"""Builds and runs tests/cpp/test_welch_mirror.cpp: the C++ host mirror of the Welch power spectra and cross spectra
(include/kofft_hip.hpp: welch / csd / set_welch_fused / welch_scale) against a direct DFT in double, route against route bit for bit,
csd(x, x) against welch(x), and the mirror's length errors, linked to libkofft_hip.so."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "tests" / "cpp" / "test_welch_mirror"


def build():
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", str(ROOT / "tests/cpp/test_welch_mirror.cpp"), "-o", str(EXE),
           f"-L{ROOT / 'kofft_amd/lib'}", "-lkofft_hip", f"-Wl,-rpath,{ROOT / 'kofft_amd/lib'}", "-Wl,-rpath,/opt/rocm/lib",
           "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)


def test_cpp_welch_mirror_compiles():
    """CPU: the header's welch / csd methods and the driver translate and link against the C ABI (no GPU needed to build)."""
    build()
    assert EXE.exists()


@pytest.mark.gpu
def test_cpp_welch_mirror_runs():
    build()
    res = subprocess.run([str(EXE)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 failed" in res.stdout
