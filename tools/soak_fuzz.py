import sys, os
os.environ.setdefault("KOFFT_HIP_HOST_PIPELINE", "0")  # one launch per call on the batch the case names (tests/conftest.py)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
os.chdir(ROOT)
import numpy as np
import test_gpu_fuzz as F
import test_gpu_rowwise_fuzz as R
import kofft_amd
from oracle import pyoracle as oracle
oracle.build()
f32 = kofft_amd.HipFftImpl(np.float32); f64 = kofft_amd.HipFftImpl(np.float64)
row32 = kofft_amd.HipFftImpl(np.float32)  # the row-wise families, route switches changing from case to case
import conftest
import spectral_oracle as SO
import test_gpu_spectral as S
from rowcheck import assert_rows_equal
spec = S.Ctx(kofft_amd.load_library())


def fuzz_spectral(seed):
    """One chirp-Z and one Goertzel case per seed: shape, parameter set, route and pointer form drawn; every row against the oracle."""
    rng = np.random.default_rng(50000 + seed)
    n, m, batch = int(rng.choice(S.CZT_NS + [500])), int(rng.choice(S.CZT_MS)), int(rng.choice(S.CZT_BATCHES))
    name = str(rng.choice(list(SO.param_sets(m))))
    form = str(rng.choice(["dev", "dev_off", "host"]))
    w, a = SO.param_sets(m)[name]
    x = rng.uniform(-1, 1, (batch, n)).astype(np.float32)
    spec.route(int(rng.integers(0, 3)))
    try:
        assert_rows_equal(S.czt_call(spec, x, m, w, a, form), SO.czt(x, m, w, a), f"czt {name} n={n} m={m} batch={batch} {form}", nan_safe=True)
    finally:
        spec.route(0)
    n, batch, nfreq = int(rng.choice(S.GZ_NS)), int(rng.choice([1, 3, 31, 85, 257, 600])), int(rng.choice([1, 3, 8, 65, 300]))
    f = rng.uniform(-1000, 9000, nfreq).astype(np.float32)
    x = rng.uniform(-1, 1, (batch, n)).astype(np.float32)
    assert_rows_equal(S.goertzel_call(spec, x, 8000.0, f, form), SO.goertzel(x, 8000.0, f), f"goertzel n={n} batch={batch} nfreq={nfreq} {form}",
                      nan_safe=True)


bad = 0
for seed in range(int(sys.argv[1]) if len(sys.argv) > 1 else 100, int(sys.argv[2]) if len(sys.argv) > 2 else 160):
    for fn, args in ((F.test_fuzz_complex.__wrapped__ if hasattr(F.test_fuzz_complex,'__wrapped__') else F.test_fuzz_complex, (f32, f64, oracle, seed)),
                     (F.test_fuzz_real, (f32, f64, oracle, seed)), (F.test_fuzz_stft, (f32, oracle, seed)),
                     (R.test_fuzz_rowwise, (row32, oracle, seed)), (fuzz_spectral, (seed,))):
        try:
            fn(*args)
        except AssertionError as e:
            bad += 1
            print("FAIL", fn.__name__, seed, e, flush=True)
print("soak done, failures:", bad)
