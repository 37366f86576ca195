"""AddressSanitizer + UBSan + LeakSanitizer over the shared host plumbing (kofft_amd/csrc/host_cache.h): the table cache (a hit returns
the first pointer and builds nothing; a failed build, a failed allocation and the failed second half of a pair leave the cache as it
was and leak nothing; a retry succeeds), the table kinds (all distinct), the grow-only scratch buffer (never shrinks, a failed growth
leaves {nullptr, 0}, a release loop frees each buffer once) and the size of a chip-resident grid.  A plain executable on a malloc / free
allocator with failure injection: the header needs no GPU and no HIP."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_host_cache_properties_under_asan_ubsan(tmp_path):
    exe = tmp_path / "host_cache_check"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, str(ROOT / "tests" / "cpp" / "host_cache_check.cpp"),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                         env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.strip().endswith("0 problems"), res.stdout
    assert "runtime error" not in res.stderr and "AddressSanitizer" not in res.stderr and "LeakSanitizer" not in res.stderr
