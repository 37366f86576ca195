"""AddressSanitizer + UBSan over the host staging layout (kofft_amd/csrc/host_layout.h): where the arrays of a host-pointer call lie
in the staging buffer, which rows a chunk of the pipelined route covers, how many rows the device routes' chunk loops take per pass
under their scratch cap (scratch_chunk_rows) and which values KOFFT_HIP_SCRATCH_CHUNK_MB accepts.  A plain executable: the header needs
no GPU and no HIP."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_host_layout_properties_under_asan_ubsan(tmp_path):
    exe = tmp_path / "host_layout_check"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, str(ROOT / "tests" / "cpp" / "host_layout_check.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip().endswith("0 problems"), res.stdout
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
