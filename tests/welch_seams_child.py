"""Run by tests/test_gpu_welch.py in a fresh process with KOFFT_HIP_SCRATCH_CHUNK_MB=1 (the knob is read when the library is loaded):
Welch power spectra and cross spectra whose chunks begin and end inside rows, on both routes, against tests/welch_oracle.py.
Prints "seams ok" and exits 0 when every row has the oracle's bytes."""
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
F = np.float32


def main() -> int:
    import kofft_amd
    import welch_oracle as wo
    from oracle import pyoracle
    from rowcheck import assert_rows_equal

    assert os.environ.get("KOFFT_HIP_SCRATCH_CHUNK_MB") == "1"
    win_len = 256
    hann = pyoracle.hann(win_len)
    rng = np.random.default_rng(26400)
    # (rows, frames, hop, the routes it is a seam case for)
    for rows, frames, hop, modes in ((5, 700, 64, (0, 1, 2)), (3, 800 * 32, 8, (2,))):
        length = (frames - 1) * hop + win_len - 3
        x = rng.standard_normal((rows, length)).astype(F)
        y = rng.standard_normal((rows, length)).astype(F)
        want = wo.welch_ref(x, hann, hop, frames, 0.3, True)
        want_c = wo.welch_ref(x, hann, hop, frames, 0.3, True, y=y)
        for mode in modes:
            f = kofft_amd.HipFftImpl(F)
            try:
                f.set_welch_fused(mode)
                for _ in range(2):
                    assert_rows_equal(f.welch_rows(x, win_len, hop, frames, None, 0.3, True), want, f"seams rows={rows} frames={frames} mode={mode}")
                    assert_rows_equal(f.csd_rows(x, y, win_len, hop, frames, None, 0.3, True), want_c, f"csd seams rows={rows} frames={frames} mode={mode}")
            finally:
                f.close()
    print("seams ok")
    return 0


if __name__ == "__main__":
    sys.exit(main())
