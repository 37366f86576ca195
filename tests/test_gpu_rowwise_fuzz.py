"""Seeded differential fuzz over the row-wise families -- DCT-II (plan_dct2), the analytic signal, the real cepstrum, the direct
DCT / DST I..IV and the wavelets -- on ONE context whose route switches change from case to case.  Each case draws a family and its
kind, a length (powers of two weighted towards the fused range 32 .. 4096 and its edges, odd and other lengths where the family takes
them, the direct tile edges, the fused-wavelet limit 16384 / 16385), a batch (1, around the kernels' rows per workgroup, around
multiples of the CU count, or random under a cap of points), a route switch, a form (host, _dev with every pointer 4 bytes off a
16-byte boundary, _dev aligned, in place where the ABI allows it) and its data (uniform, or with special-value rows).  Every row of
every output is compared bit for bit with the family's oracle (NaN-safe), every call runs twice and must give the same bytes, and
finite cases are also held to the float64 definitions within the CPU tests' bounds (DCT-II past 2048 points: a measured one,
see _float64_check).  A failure names the case."""
import numpy as np
import pytest

import wavelet_oracle as wo
from cepstrum_oracle import cepstrum_ref
from dct_oracle import dct2_ref
from hilbert_oracle import hilbert_ref
from rowcheck import assert_rows_equal
from trig_direct_oracle import direct, direct_f64

pytestmark = pytest.mark.gpu

F = np.float32
CUS = 256                 # MI355X compute units: the persistent kernels' grid
MAX_POINTS = 1 << 21      # per case, in + out
DIRECT_TERMS = 1 << 26    # batch * n * n of a direct case (the C oracle's cost)
WAVELET_INV_ROWS = 64     # rows of a wavelet inverse case (the oracle's tail loop is in Python)
SPECIALS = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1.2e-38, 3e38, -3e38, np.inf, -np.inf, np.nan], F)
FAMILIES = ["dct2", "hilbert", "cepstrum", "direct", "wavelet"]
DIRECT_EDGES = [63, 64, 65, 127, 128, 129]
# float64 relative error of plan_dct2 at n = 2^k, k >= 12 (see _float64_check)
DCT2_POW2_ERR = {12: 8.87e-5, 13: 3.70e-5, 14: 4.26e-4, 15: 1.05e-3, 16: 5.64e-4, 17: 3.01e-4, 18: 1.58e-4, 19: 5.16e-5, 20: 1.18e-4}


def _pow2_len(rng, lo=0, hi=20):
    """A power of two 2^lo .. 2^hi, two thirds of the time inside the fused range 32 .. 4096 (edges included)."""
    if rng.random() < 0.67:
        return 1 << int(rng.integers(max(lo, 5), min(hi, 12) + 1))
    return 1 << int(rng.integers(lo, hi + 1))


def _length(rng, fam):
    r = rng.random()
    if fam in ("hilbert", "cepstrum"):
        return _pow2_len(rng)
    if fam == "direct":
        if r < 0.35:
            return int(rng.choice(DIRECT_EDGES))
        if r < 0.6:
            return _pow2_len(rng, 0, 12)
        return int(rng.integers(1, 4097 if rng.random() < 0.3 else 600))
    if fam == "dct2":
        if r < 0.45:
            return _pow2_len(rng)
        if r < 0.7:
            return int(rng.integers(1, 200)) | 1  # odd
        return int(rng.integers(2, 1 << int(rng.integers(8, 21))))
    # wavelet
    if r < 0.3:
        return _pow2_len(rng, 0, 20)
    if r < 0.45:
        return int(rng.choice([16383, 16384, 16385, 10923, 12000]))
    if r < 0.65:  # odd intermediates: a multiple of 2^k plus an odd part
        return (int(rng.integers(1, 40)) | 1) << int(rng.integers(0, 6)) | int(rng.integers(0, 2))
    return int(rng.integers(1, 1 << int(rng.integers(4, 19))))


def _batch(rng, fam, n, cap_points):
    cap = max(1, cap_points // max(n, 1))
    r = rng.random()
    if r < 0.15:
        return 1
    if fam == "direct":
        cap = min(cap, max(1, DIRECT_TERMS // max(n * n, 1)))
        edges = [127, 128, 129, 63, 64, 65]
    elif fam == "wavelet":
        edges = [max(1, 1024 // max(n, 1) + d) for d in (-1, 0, 1)] + [max(1, 8192 // max(n, 1) + d) for d in (-1, 0, 1)]
    else:
        edges = [CUS * k + d for k in (1, 2, 4, 8) for d in (-1, 0, 1)]
    edges = [b for b in edges if b <= cap]
    if r < 0.7 and edges:
        return int(rng.choice(edges))
    return int(rng.integers(1, cap + 1))


def _data(rng, shape, specials):
    x = rng.uniform(-1, 1, shape).astype(F)
    if specials and x.size:
        b, n = shape
        for r in rng.choice(b, size=min(b, 1 + int(rng.integers(0, 4))), replace=False):
            kind = int(rng.integers(0, 3))
            if kind == 0:  # a whole row of one special value
                x[r] = rng.choice(SPECIALS)
            elif kind == 1:  # a few specials in a uniform row
                pos = rng.choice(n, size=min(n, 1 + int(rng.integers(0, 3))), replace=False)
                x[r, pos] = rng.choice(SPECIALS, size=pos.size)
            else:  # a row of specials
                x[r] = rng.choice(SPECIALS, size=n)
    return x


def _padding_holds(torch, t, off, floats, fill):
    pad = torch.cat([t[:off], t[off + floats:]])
    assert bool((pad == fill).all()), f"the padding around a {floats}-float device buffer was written (fill {fill})"


class Dev:
    """Device copies of host arrays at a chosen float offset from a 16-byte aligned allocation."""

    def __init__(self, off):
        import torch

        self.torch, self.off, self.keep, self.fill = torch, off, [], {}

    def put(self, a):
        t = self.torch.zeros(a.size + self.off + 4, dtype=self.torch.float32, device="cuda")
        t[self.off:self.off + a.size] = self.torch.from_numpy(np.ascontiguousarray(a, F).reshape(-1).view(F)).cuda()
        self.keep.append(t)
        self.fill[id(t)] = 0.0
        # torch fills and copies on its own stream, the library runs on the context's: both must be done before the call
        self.torch.cuda.synchronize()
        return t.data_ptr() + 4 * self.off

    def empty(self, floats, fill=7.0):
        t = self.torch.full((floats + self.off + 4,), fill, dtype=self.torch.float32, device="cuda")
        self.keep.append(t)
        self.fill[id(t)] = fill
        self.torch.cuda.synchronize()
        return t.data_ptr() + 4 * self.off, t

    def check_padding(self, t, floats):
        """The floats in front of and behind the `floats` the call may write still hold the allocation's fill value."""
        _padding_holds(self.torch, t, self.off, floats, self.fill[id(t)])

    def get(self, t, floats):
        self.torch.cuda.synchronize()
        self.check_padding(t, floats)
        return t[self.off:self.off + floats].cpu().numpy()


def _twice(fn, what=""):
    a = fn()
    b = fn()
    pa = a if isinstance(a, (tuple, list)) else (a,)
    pb = b if isinstance(b, (tuple, list)) else (b,)
    for u, v in zip(pa, pb):
        if isinstance(u, list):
            assert [np.asarray(p).tobytes() for p in u] == [np.asarray(q).tobytes() for q in v], f"{what}: two runs of the same call differ"
        else:
            assert np.asarray(u).tobytes() == np.asarray(v).tobytes(), f"{what}: two runs of the same call differ"
    return a


# ---- one case per family -------------------------------------------------------------------------------------------------------

def _rowwise_call(f, fam, kind, x, form):
    """dct2 / hilbert / cepstrum / direct through `form`: the output array (host layout)."""
    b, n = x.shape
    out_floats = b * n * (2 if fam == "hilbert" else 1)
    out_dt = np.complex64 if fam == "hilbert" else F
    if form == "host":
        if fam == "direct":
            fam_, t = kind
            return (f.dct_direct_batch if fam_ == "dct" else f.dst_direct_batch)(x, t)
        return {"dct2": f.dct2_batch, "hilbert": f.hilbert_batch, "cepstrum": f.cepstrum_batch}[fam](x)
    if form == "inplace":
        buf = x.copy()
        if fam == "cepstrum":
            f._check(f._lib.kofft_hip_cepstrum_f32(f._ctx, buf.ctypes.data, buf.ctypes.data, n, b))
        else:
            fam_, t = kind
            fn = f._lib.kofft_hip_dct_direct_f32 if fam_ == "dct" else f._lib.kofft_hip_dst_direct_f32
            f._check(fn(f._ctx, t, buf.ctypes.data, buf.ctypes.data, n, b))
        return buf
    if form == "dev_inplace":  # cepstrum only: d_in == d_out
        dv = Dev(1)
        p = dv.put(x)
        f.cepstrum_dev(p, p, n, b)
        return dv.get(dv.keep[-1], b * n).reshape(b, n)
    dv = Dev(1 if form == "dev_off" else 0)
    d_in = dv.put(x)
    # the analytic signal's complex output must be 8-byte aligned (include/kofft_hip.h): only its input is moved off
    d_out, t_out = (Dev(0) if fam == "hilbert" else dv).empty(out_floats)
    if fam == "direct":
        fam_, t = kind
        (f.dct_direct_dev if fam_ == "dct" else f.dst_direct_dev)(t, d_in, d_out, n, b)
    else:
        getattr(f, f"{fam}_dev")(d_in, d_out, n, b)
    off = 0 if fam == "hilbert" else dv.off
    import torch

    torch.cuda.synchronize()
    _padding_holds(torch, t_out, off, out_floats, 7.0)
    return t_out[off:off + out_floats].cpu().numpy().view(out_dt).reshape(b, n)


def _rowwise_oracle(fam, kind, x):
    if fam == "dct2":
        return dct2_ref(x)
    if fam == "hilbert":
        return hilbert_ref(x)
    if fam == "cepstrum":
        return cepstrum_ref(x)
    from oracle import pyoracle

    fam_, t = kind
    return direct(fam_, t, x) if x.shape[1] <= 64 else pyoracle.direct_mt(fam_, t, x)


def _rel_l2(got, want):
    den = float(np.linalg.norm(want))
    return float(np.linalg.norm(got - want)) / den if den else float(np.linalg.norm(got))


def _float64_check(fam, kind, x, got, what):
    """The float64 definitions, with the CPU tests' bounds (a few rows: this checks the oracle's reading, not every row again)."""
    x = x[:8].astype(np.float64)
    got = got[:8]
    n = x.shape[1]
    if fam == "dct2":
        import scipy.fft

        want = scipy.fft.dct(x, type=2, axis=-1) / 2.0  # scipy's unnormalised DCT-II is 2 * sum x cos(..)
        # test_dct_tables.py's 2e-6 * max(1, log2 n) holds for powers of two up to 2048.  Beyond, the reference's twiddle recurrence
        # adds an error that is nearly the same for every row of a given n but does not grow steadily with it: DCT2_POW2_ERR, measured on
        # the CPU oracle (the device's bytes), 4 seeds x 8 uniform rows, spread under 1 %.  The bound is 2.5x that.  Other n run the
        # 2n-point rfft through Bluestein (two transforms of m >= 4n - 1 points and a chirp product), the reference's own error: 5.6e-5
        # at 1000, 1.05e-3 at 5000, 2.9e-3 at 12345, 5.9e-2 at 1000001, at most 2.3e-7 * n, hence 1e-6 + 5e-7 * n.
        lg = int(n).bit_length() - 1
        if n & (n - 1) == 0:
            bound = 2.5 * DCT2_POW2_ERR[lg] if lg in DCT2_POW2_ERR else 2e-6 * max(1.0, lg)
        else:
            bound = 1e-6 + 5e-7 * n
        err = _rel_l2(got.astype(np.float64), want)
        assert err <= bound, f"{what}: float64 rel err {err:.2e} > {bound:.2e}"
    elif fam == "hilbert":
        from scipy.signal import hilbert

        err = _rel_l2(got.astype(np.complex128), hilbert(x, axis=-1))
        assert err <= 1e-7 + 1e-7 * n, f"{what}: float64 rel err {err:.2e}"  # test_hilbert_cpu.py
    elif fam == "cepstrum":
        want = np.fft.ifft(np.log(np.abs(np.fft.fft(x, axis=-1)) + 1e-12), axis=-1).real
        err = _rel_l2(got.astype(np.float64), want)
        assert err <= 1e-6 + 2e-7 * n, f"{what}: float64 rel err {err:.2e}"  # test_cepstrum_cpu.py
    elif fam == "direct" and n <= 1024:
        fam_, t = kind
        want, mag = direct_f64(fam_, t, x)
        bound = (n + 4) * np.finfo(F).eps * (mag + 1e-30) * 2  # test_trig_direct_cpu.py
        assert np.all(np.abs(got.astype(np.float64) - want) <= bound), f"{what}: beyond the float64 bound"


def _wavelet_case(f, rng, name, n, b, inverse, levels, form, specials, what):
    with np.errstate(all="ignore"):
        if not inverse:
            x = _data(rng, (b, n), specials)
            if levels is None:
                if form == "host":
                    a, d = _twice(lambda: f.dwt_batch(x, name), what)
                else:
                    dv = Dev(1 if form == "dev_off" else 0)
                    h = n // 2
                    pa, ta = dv.empty(b * h)
                    pd, td = dv.empty(b * h)
                    px = dv.put(x)
                    f.dwt_dev(name, px, pa, pd, n, b)
                    a, d = dv.get(ta, b * h).reshape(b, h), dv.get(td, b * h).reshape(b, h)
                    f.dwt_dev(name, px, pa, pd, n, b)
                    assert dv.get(ta, b * h).tobytes() == a.tobytes() and dv.get(td, b * h).tobytes() == d.tobytes(), f"{what}: two runs differ"
                wa, wd = wo.forward(name, x)
                assert_rows_equal(a, wa, what + " approx", nan_safe=True)
                assert_rows_equal(d, wd, what + " detail", nan_safe=True)
                return
            lens = wo.multi_lengths(n, levels)
            if form == "host":
                a, ds = _twice(lambda: f.wavedec_batch(x, name, levels), what)
            else:
                dv = Dev(1 if form == "dev_off" else 0)
                px = dv.put(x)
                pa, ta = dv.empty(b * lens[-1])
                tot = sum(lens[1:])
                pd, td = dv.empty(max(1, b * tot))
                f.wavedec_dev(name, px, pa, pd if levels else 0, n, b, levels)
                a, packed = dv.get(ta, b * lens[-1]).reshape(b, lens[-1]), dv.get(td, b * tot)
                f.wavedec_dev(name, px, pa, pd if levels else 0, n, b, levels)
                assert dv.get(ta, b * lens[-1]).tobytes() == a.tobytes() and dv.get(td, b * tot).tobytes() == packed.tobytes(), \
                    f"{what}: two runs differ"
                ds, o = [], 0
                for m in lens[1:]:
                    ds.append(packed[o:o + b * m].reshape(b, m))
                    o += b * m
            wa, wds = wo.forward_multi(name, x, levels)
            assert_rows_equal(a, wa, what + " approx", nan_safe=True)
            assert len(ds) == levels
            for l, (g, w) in enumerate(zip(ds, wds)):
                assert_rows_equal(g, w, f"{what} detail {l}", nan_safe=True)
            return
        if levels is None:  # single level: idwt on rows of h approximations and h details
            h = max(1, n // 2)
            ap, dt = _data(rng, (b, h), specials), _data(rng, (b, h), specials)
            if form == "host":
                got = _twice(lambda: f.idwt_batch(ap, dt, name), what)
            else:
                dv = Dev(1 if form == "dev_off" else 0)
                pa, pd = dv.put(ap), dv.put(dt)
                po, to = dv.empty(2 * b * h)
                f.idwt_dev(name, pa, pd, po, h, b)
                got = dv.get(to, 2 * b * h).reshape(b, 2 * h)
                f.idwt_dev(name, pa, pd, po, h, b)
                assert dv.get(to, 2 * b * h).tobytes() == got.tobytes(), f"{what}: two runs differ"
            assert_rows_equal(got, wo.inverse(name, ap, dt), what, nan_safe=True)
            return
        # multi level: n0 approximations folded with details of the lengths the forward would give (+ an ignored extra sample at times)
        n0 = max(1, n >> levels)
        dl = [(n0 << (levels - 1 - l)) + int(rng.integers(0, 2)) for l in range(levels)]
        ap = _data(rng, (b, n0), specials)
        dets = [_data(rng, (b, m), specials) for m in dl]
        want = wo.inverse_multi(name, ap, dets)
        if form == "host":
            got = _twice(lambda: f.waverec_batch(ap, dets, name), what)
        else:
            dv = Dev(1 if form == "dev_off" else 0)
            pa = dv.put(ap)
            pd = dv.put(np.concatenate([d.ravel() for d in dets])) if dets else 0  # levels == 0: no details (may be null)
            total = n0 << levels
            po, to = dv.empty(b * total)
            f.waverec_dev(name, pa, pd, dl, po, n0, b)
            got = dv.get(to, b * total).reshape(b, total)
            f.waverec_dev(name, pa, pd, dl, po, n0, b)
            assert dv.get(to, b * total).tobytes() == got.tobytes(), f"{what}: two runs differ"
        assert_rows_equal(got, want, what, nan_safe=True)


@pytest.fixture(scope="module")
def ctx():
    """One context for every case of the module: the route switches change between cases, tables and scratch are shared."""
    import kofft_amd

    f = kofft_amd.HipFftImpl(np.float32)
    yield f
    f.close()


@pytest.mark.parametrize("seed", range(16))
def test_fuzz_rowwise(ctx, oracle, seed):
    rng = np.random.default_rng(21000 + seed)
    f = ctx
    for case in range(12):
        fam = FAMILIES[int(rng.integers(0, len(FAMILIES)))]
        specials = bool(rng.random() < 0.25)
        if fam == "wavelet":
            name = wo.NAMES[int(rng.integers(0, len(wo.NAMES)))]
            n = _length(rng, fam)
            inverse = bool(rng.random() < 0.4)
            r = rng.random()
            if r < 0.3:
                levels = None  # single level
            else:
                deep = max(1, int(n - 1).bit_length())  # the level at which the length reaches 1
                levels = int(rng.choice([0, 1, 2, 3, deep, deep + 2])) if r < 0.85 else int(rng.integers(0, deep + 3))
            if inverse:
                n = min(n, 1 << 16)
            b = _batch(rng, fam, n, MAX_POINTS // (3 if inverse else 2))
            if inverse:
                b = min(b, WAVELET_INV_ROWS)
            mode = int(rng.integers(0, 3))
            form = ["host", "dev_off", "dev"][int(rng.integers(0, 3))]
            what = (f"seed={seed} case={case}: wavelet {name} {'inverse' if inverse else 'forward'} levels={'single' if levels is None else levels} n={n} batch={b} "
                    f"fused={mode} form={form} specials={specials}")
            f.set_wavelet_fused(mode)
            _wavelet_case(f, rng, name, n, b, inverse, levels, form, specials, what)
            continue
        n = _length(rng, fam)
        kind = None
        forms = ["host", "dev_off", "dev"]
        if fam == "direct":
            kind = (("dct", "dst")[int(rng.integers(0, 2))], int(rng.integers(1, 5)))
            routed = bool(rng.random() < 0.6)
            f.set_direct_tiled(routed)
            forms.append("inplace")
        elif fam == "cepstrum":
            routed = bool(rng.random() < 0.6)
            f.set_cepstrum_fused(routed)
            forms += ["inplace", "dev_inplace"]
        elif fam == "hilbert":
            routed = bool(rng.random() < 0.6)
            f.set_hilbert_fused(routed)
        else:
            routed = bool(rng.random() < 0.6)
            f.set_dct_fused(routed)
        b = _batch(rng, fam, n, MAX_POINTS // (3 if fam == "hilbert" else 2))
        form = forms[int(rng.integers(0, len(forms)))]
        what = (f"seed={seed} case={case}: {fam}{'' if kind is None else ' %s%d' % kind} n={n} batch={b} route_on={routed} form={form} "
                f"specials={specials}")
        x = _data(rng, (b, n), specials)
        with np.errstate(all="ignore"):
            got = _twice(lambda: _rowwise_call(f, fam, kind, x, form), what)
            assert_rows_equal(got, _rowwise_oracle(fam, kind, x), what, nan_safe=True)
        if not specials:
            _float64_check(fam, kind, x, got, what)
    for on in (f.set_dct_fused, f.set_hilbert_fused, f.set_cepstrum_fused, f.set_direct_tiled):
        on(True)
    f.set_wavelet_fused(1)
