"""AddressSanitizer + UBSan over the walk arithmetic of the 4096-point c32 streaming kernel (kofft_amd/csrc/persist_walk.h): the
direction rule's table, keep_from and the mirrored row at batches up to 2^40, and the mirrored row as a permutation for seeded
(batch, split) pairs -- tests/cpp/sanitize_persist_walk.cpp, a stand-alone program run on the CPU."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_the_walk_arithmetic_under_asan_ubsan(tmp_path):
    exe = tmp_path / "sanitize_persist_walk"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *flags, str(ROOT / "tests" / "cpp" / "sanitize_persist_walk.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert res.returncode == 0, res.stdout + res.stderr
    assert "4000 (batch, split) pairs, 0 problems" in res.stdout
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr
