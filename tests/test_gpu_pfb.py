"""The polyphase filter bank of DESIGN.md 5.34 on the device, bit for bit against tests/pfb_oracle.py.  M = 32 .. 4096 a power of two
has pfb_fused_kernel<5 .. 12> (one launch per analysis; the default up to M = 1024, set_pfb_fused(2) beyond) and
pfb_inverse_fused_kernel<5 .. 12> (one per chunk of the synthesis); every other M -- and every M in a context with set_pfb_fused(False)
-- runs pfb_fold_kernel -> fft_dev (-> pfb_prefix_kernel) and pfb_complete_kernel -> inverse fft_dev -> pfb_real_kernel through the
context's scratch.  The synthesis adds pfb_ola_kernel.  Every device call runs twice and its two results are compared; the default
context, the composed one and one with the fused kernels wherever they exist get the same inputs and must give the same bytes.  The oracle is computed once per geometry, with all M bins, and the kept bins are its prefix."""
import numpy as np
import pytest

from conftest import bits_equal, seeded
import pfb_oracle as po
from rowcheck import assert_rows_equal
from test_pfb_cpu import sine_pair

pytestmark = pytest.mark.gpu
F = np.float32
XPB = {5: 32, 6: 16, 7: 16, 8: 16, 9: 4, 10: 4, 11: 2, 12: 1}  # items per workgroup of the fused kernels, by log2 M
FUSED_M = [32 << i for i in range(8)]
COMPOSED_M = [1, 2, 4, 8, 16, 6, 240, 400, 8192, 16384]


@pytest.fixture(scope="module")
def routes(fft32):
    """The default context (the measured choice), one with the fused route off (set_pfb_fused(False): every call through the composed
    route) and one with set_pfb_fused(2) (the fused kernels wherever they exist)."""
    import kofft_amd

    composed, forced = kofft_amd.HipFftImpl(F), kofft_amd.HipFftImpl(F)
    composed.set_pfb_fused(False)
    forced.set_pfb_fused(2)
    yield [(fft32, "default route"), (composed, "composed route"), (forced, "fused wherever it exists")]
    composed.close()
    forced.close()


def _up(a, off=0, fill=0.0):
    import torch

    a = np.ascontiguousarray(a)
    if a.dtype.kind == "c":
        a = a.view(F)
    a = np.ascontiguousarray(a, F)
    d = torch.full((a.size + off,), fill, dtype=torch.float32, device="cuda")
    d[off:] = torch.from_numpy(a.reshape(-1)).cuda()
    return d


def _analysis_dev(f, x, h, m, hop, lead, frames, bins, stride=None, off=0):
    """x: [rows, nx]; stride > nx: the gaps between the rows (and behind the last) hold NaN.  off: x and h lie `off` floats into
    their allocations (still 4-byte aligned)."""
    import torch

    rows, nx = x.shape
    stride = nx if stride is None else stride
    padded = np.full((rows, stride), np.nan, F)
    padded[:, :nx] = x
    dx, dh = _up(padded, off, fill=float("nan")), _up(h, off)
    res = []
    for _ in range(2):
        out = torch.full((rows * frames * bins * 2,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # (the context's stream does not wait for torch's)
        f.pfb_analysis_dev(dx.data_ptr() + 4 * off, rows, nx, stride, dh.data_ptr() + 4 * off, h.size, m, hop, lead, out.data_ptr(), frames, bins)
        f.synchronize()
        res.append(out.cpu().numpy().view(np.complex64).reshape(rows, frames, bins))
    assert bits_equal(res[0], res[1]), "pfb_analysis_dev: two runs of the same call differ"
    return res[0]


def _synthesis_dev(f, S, g, m, hop, scale, first, count):
    import torch

    rows, frames, bins = S.shape
    dS, dg = _up(S), _up(g)
    res = []
    for _ in range(2):
        out = torch.full((rows * count,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # (the context's stream does not wait for torch's)
        f.pfb_synthesis_dev(dS.data_ptr(), rows, frames, bins, dg.data_ptr(), g.size, m, hop, scale, out.data_ptr(), first, count)
        f.synchronize()
        res.append(out.cpu().numpy().reshape(rows, count))
    assert bits_equal(res[0], res[1]), "pfb_synthesis_dev: two runs of the same call differ"
    return res[0]


def _both(routes, run, want, what, nan_safe=False):
    first = None
    for f, name in routes:
        got = run(f)
        assert_rows_equal(got.reshape(want.shape[0], -1), want.reshape(want.shape[0], -1), f"{what}: {name}", nan_safe=nan_safe)
        if first is None:
            first = got
        elif not nan_safe:
            assert bits_equal(got, first), f"{what}: {name} differs from the default route"


def _covering(nx, lead, hop):
    """frames f with f D - lead < nx: the count that covers the row"""
    return -(-(nx + lead) // hop)


def _bins_forms(m):
    return sorted({m, m // 2 + 1, 1, min(5, m)})


# ---- analysis ------------------------------------------------------------------------------------------------------------------------
def _analysis_ladder(routes, m, taps_list, seed):
    rows = 3
    xpb = XPB.get(m.bit_length() - 1, 1) if m & (m - 1) == 0 and 32 <= m <= 4096 else 1
    for taps in taps_list:
        nh = taps * m
        rng = seeded(seed + 10 * m + taps)
        h = rng.uniform(0.1, 1, nh).astype(F)
        hops = sorted({m, max(m // 2, 1), max(m - 3, 1), m + 7})
        for hop in hops:
            for lead in sorted({0, max(nh - hop, 0), nh - 1}):
                nx = nh + 2 * m + 5
                frames = _covering(nx, lead, hop) + 2
                while xpb > 1 and (rows * frames) % xpb == 0:  # the last workgroup partly empty: one more hop of samples, one more frame
                    nx += hop
                    frames = _covering(nx, lead, hop) + 2
                x = rng.uniform(-1, 1, (rows, nx)).astype(F)
                full = po.analysis_ref(x, h, m, hop, lead, frames, m)
                assert not full[:, -2:].any()  # the two frames past the row's end are exactly zero
                for bins in _bins_forms(m):
                    want = np.ascontiguousarray(full[:, :, :bins])
                    what = f"pfb analysis M={m} T={taps} D={hop} lead={lead} nx={nx} frames={frames} bins={bins}"
                    _both(routes, lambda f: _analysis_dev(f, x, h, m, hop, lead, frames, bins, nx + 5), want, what + " dev")
                if hop == hops[0] and lead == 0:  # the host form, one-sided and full
                    for bins in (m // 2 + 1, m):
                        want = np.ascontiguousarray(full[:, :, :bins])
                        _both(routes, lambda f: f.pfb_analysis(x, h, m, hop, lead, frames, bins), want,
                              f"pfb analysis M={m} T={taps} D={hop} bins={bins} host")


@pytest.mark.parametrize("m", FUSED_M)
def test_analysis_fused_ladder(fft32, routes, oracle, m):
    """3 rows a stride apart with NaN between them; T 1 and 3; hops M, M/2, M - 3, M + 7; leads 0, nh - D, nh - 1; two frames past the
    row's end; every form of bins; rows * frames no multiple of XPB, so row seams fall inside workgroups and the last one is ragged."""
    _analysis_ladder(routes, m, (1, 3), 15000)


@pytest.mark.parametrize("m", COMPOSED_M)
def test_analysis_composed_lengths(fft32, routes, oracle, m):
    _analysis_ladder(routes, m, (1, 3) if m <= 400 else (2,), 15100)


@pytest.mark.parametrize("m", [64, 4096])
def test_analysis_buffers_inside_allocations_and_off_alignment(fft32, routes, oracle, m):
    """x and h one float into their allocations (4-byte aligned: still the fused route); then x two bytes into its allocation, which
    takes the composed route on the default context and gives the same bytes."""
    import torch

    taps, hop, lead, rows = 3, m // 2, m, 3
    nh = taps * m
    rng = seeded(15200 + m)
    nx = 4 * m + 3
    frames = _covering(nx, lead, hop) + 1
    x = rng.uniform(-1, 1, (rows, nx)).astype(F)
    h = rng.uniform(0.1, 1, nh).astype(F)
    bins = m // 2 + 1
    want = po.analysis_ref(x, h, m, hop, lead, frames, bins)
    _both(routes, lambda f: _analysis_dev(f, x, h, m, hop, lead, frames, bins, nx + 1, off=1), want, f"pfb analysis M={m} off=1")
    raw = torch.zeros(x.nbytes + 8, dtype=torch.uint8, device="cuda")
    raw[2:2 + x.nbytes] = torch.from_numpy(x.reshape(-1).view(np.uint8)).cuda()
    dh = _up(h)
    out = torch.full((rows * frames * bins * 2,), float("nan"), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # (the context's stream does not wait for torch's)
    fft32.pfb_analysis_dev(raw.data_ptr() + 2, rows, nx, nx, dh.data_ptr(), nh, m, hop, lead, out.data_ptr(), frames, bins)
    fft32.synchronize()
    got = out.cpu().numpy().view(np.complex64).reshape(rows, -1)
    assert_rows_equal(got, want.reshape(rows, -1), f"pfb analysis M={m} input off 4-byte alignment")


def test_analysis_seam_inside_workgroups(fft32, routes, oracle):
    """M = 64: 16 items per workgroup, 7 frames per row, 11 rows: every workgroup holds items of two or three rows."""
    m, taps, hop, lead, rows, nx, frames = 64, 4, 48, 100, 11, 300, 7
    rng = seeded(15300)
    x = rng.uniform(-1, 1, (rows, nx)).astype(F)
    h = rng.uniform(0.1, 1, taps * m).astype(F)
    want = po.analysis_ref(x, h, m, hop, lead, frames, 33)
    _both(routes, lambda f: _analysis_dev(f, x, h, m, hop, lead, frames, 33, nx + 1), want, "pfb analysis row seams")


def test_analysis_composed_across_scratch_seams(oracle, monkeypatch):
    """KOFFT_HIP_SCRATCH_CHUNK_MB=1 at M = 16384: 8 items per chunk; 3 rows x 7 frames, so seams fall inside rows and row starts
    inside chunks; the one-sided form (the prefix copy) and the full one (the transform straight into the output)."""
    import kofft_amd

    monkeypatch.setenv("KOFFT_HIP_SCRATCH_CHUNK_MB", "1")
    f = kofft_amd.HipFftImpl(F)
    try:
        m, taps, rows, frames = 16384, 2, 3, 7
        nx = 5 * m + 77
        rng = seeded(15400)
        x = rng.uniform(-1, 1, (rows, nx)).astype(F)
        h = rng.uniform(0.1, 1, taps * m).astype(F)
        full = po.analysis_ref(x, h, m, m, m, frames, m)
        for bins in (m // 2 + 1, m):
            got = _analysis_dev(f, x, h, m, m, m, frames, bins, nx + 5)
            assert_rows_equal(got.reshape(rows, -1), np.ascontiguousarray(full[:, :, :bins]).reshape(rows, -1), f"pfb analysis seams bins={bins}")
    finally:
        f.close()


@pytest.mark.parametrize("m", [64, 240])
def test_analysis_special_values(fft32, routes, oracle, m):
    """A NaN and an Inf sample reach exactly the frames whose term sets hold them: those frames are non-finite in every bin, every
    other frame is finite, and everything equals the oracle."""
    taps, hop, lead, rows = 3, m // 2, m // 4, 3
    nh = taps * m
    rng = seeded(15500 + m)
    nx = 4 * nh
    frames = _covering(nx, lead, hop)
    x = rng.uniform(-1, 1, (rows, nx)).astype(F)
    h = rng.uniform(0.1, 1, nh).astype(F)
    where = {0: (5, np.nan), 1: (nx // 2, np.inf), 2: (nx - 1, -np.inf)}
    for r, (s, v) in where.items():
        x[r, s] = v
    want = po.analysis_ref(x, h, m, hop, lead, frames, m)
    for f, _ in routes:
        got = _analysis_dev(f, x, h, m, hop, lead, frames, m)
        assert_rows_equal(got.reshape(rows, -1), want.reshape(rows, -1), f"pfb analysis M={m} special values", nan_safe=True)
        for r, (s, _) in where.items():
            fr = np.arange(frames)
            holds = (fr * hop - lead <= s) & (s < fr * hop - lead + nh)
            assert holds.any() and not holds.all()
            bad = ~np.isfinite(got[r].real) | ~np.isfinite(got[r].imag)
            assert bad[holds].all() and not bad[~holds].any(), (m, r)


@pytest.mark.parametrize("m,hop", [(64, 24), (1024, 512), (240, 100), (8192, 8192)])
def test_one_tap_per_channel_is_the_stft(fft32, routes, oracle, m, hop):
    """T = 1, lead = 0: the bytes of stft_rows and of stft_onesided with window h and hop D."""
    rng = seeded(15600 + m)
    rows, nx = 3, 5 * m + 7
    x = rng.uniform(-1, 1, (rows, nx)).astype(F)
    h = rng.uniform(0.1, 1, m).astype(F)
    frames = -(-nx // hop)
    full = fft32.stft_rows(x, h, hop, frames)
    half = fft32.stft_onesided(x, h, hop, frames)
    for f, _ in routes:
        assert bits_equal(f.pfb_analysis(x, h, m, hop, 0, frames, m), full)
        assert bits_equal(f.pfb_analysis(x, h, m, hop, 0, frames, m // 2 + 1), half)


# ---- synthesis -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", FUSED_M + COMPOSED_M)
def test_synthesis_ladder_and_windows(fft32, routes, oracle, m):
    """3 rows x 6 frames, both forms of bins, hops M, M/2 and M - 3; the whole of `full`, windows that start and end inside hop blocks,
    one inside block 0, the last sample."""
    rows, frames = 3, 6
    taps = 3 if m <= 4096 else 2
    nh = taps * m
    rng = seeded(15700 + m)
    g = rng.uniform(0.1, 1, nh).astype(F)
    scale = 0.75
    for bins in sorted({m, m // 2 + 1} if m % 2 == 0 else {m}):
        S = (rng.uniform(-1, 1, (rows, frames, bins)) + 1j * rng.uniform(-1, 1, (rows, frames, bins))).astype(np.complex64)
        for hop in sorted({m, max(m // 2, 1), max(m - 3, 1)}):
            full = po.synthesis_ref(S, g, m, hop, scale)
            n = full.shape[1]
            q = max(hop // 4, 1)
            windows = [(0, n), (min(hop + q, n - 1), max(min(2 * hop + 1, n - hop - q), 1)), (0, q), (n - 1, 1)]
            for first, count in windows:
                want = np.ascontiguousarray(full[:, first:first + count])
                what = f"pfb synthesis M={m} bins={bins} D={hop} window=({first}, {count})"
                _both(routes, lambda f: _synthesis_dev(f, S, g, m, hop, scale, first, count), want, what + " dev")
            if hop == m:
                _both(routes, lambda f: f.pfb_synthesis(S, g, m, hop, scale), full, f"pfb synthesis M={m} bins={bins} host")


def test_synthesis_hop_beyond_the_taps(fft32, routes, oracle):
    """D > nh: the samples between two frames are covered by none and are exactly +0."""
    m, hop, rows, frames = 64, 100, 3, 5
    rng = seeded(15800)
    g = rng.uniform(0.1, 1, m).astype(F)
    S = (rng.uniform(-1, 1, (rows, frames, 33)) + 1j * rng.uniform(-1, 1, (rows, frames, 33))).astype(np.complex64)
    full = po.synthesis_ref(S, g, m, hop, -2.0)
    assert not full[:, m:hop].any() and not np.signbit(full[:, m:hop]).any()
    _both(routes, lambda f: _synthesis_dev(f, S, g, m, hop, -2.0, 0, full.shape[1]), full, "pfb synthesis D > nh")


@pytest.mark.parametrize("fused", [True, False])
def test_synthesis_across_scratch_seams(oracle, monkeypatch, fused):
    """KOFFT_HIP_SCRATCH_CHUNK_MB=1 at M = 1024: 256 (fused) or 128 (composed) frames per chunk; 3 rows x 200 frames, T = 2 and D =
    M / 2, so seams fall inside rows, where a chunk recomputes the ceil(nh / D) - 1 = 3 frames before its first, and row starts fall
    inside chunks.  Also a window that leaves out whole chunks."""
    import kofft_amd

    monkeypatch.setenv("KOFFT_HIP_SCRATCH_CHUNK_MB", "1")
    f = kofft_amd.HipFftImpl(F)
    try:
        f.set_pfb_fused(fused)
        m, taps, rows, frames = 1024, 2, 3, 200
        hop, bins = m // 2, m // 2 + 1
        rng = seeded(15900)
        g = rng.uniform(0.1, 1, taps * m).astype(F)
        S = (rng.uniform(-1, 1, (rows, frames, bins)) + 1j * rng.uniform(-1, 1, (rows, frames, bins))).astype(np.complex64)
        full = po.synthesis_ref(S, g, m, hop, 0.5)
        assert_rows_equal(_synthesis_dev(f, S, g, m, hop, 0.5, 0, full.shape[1]), full, f"pfb synthesis seams fused={fused}")
        first, count = 57 * hop + 100, 100 * hop
        assert_rows_equal(_synthesis_dev(f, S, g, m, hop, 0.5, first, count), np.ascontiguousarray(full[:, first:first + count]),
                          f"pfb synthesis seams window fused={fused}")
    finally:
        f.close()


@pytest.mark.parametrize("m", [64, 240])
def test_synthesis_special_values(fft32, routes, oracle, m):
    """A NaN in one frame and an Inf in another reach exactly the samples those frames cover."""
    taps, hop, rows, frames = 2, m // 2, 2, 8
    nh = taps * m
    rng = seeded(16000 + m)
    g = rng.uniform(0.1, 1, nh).astype(F)
    S = (rng.uniform(-1, 1, (rows, frames, m)) + 1j * rng.uniform(-1, 1, (rows, frames, m))).astype(np.complex64)
    S[0, 2, 3] = np.nan
    S[1, 5, m - 1] = complex(np.inf, -np.inf)
    full = po.synthesis_ref(S, g, m, hop, 1.0)
    for f, _ in routes:
        got = _synthesis_dev(f, S, g, m, hop, 1.0, 0, full.shape[1])
        assert_rows_equal(got, full, f"pfb synthesis M={m} special values", nan_safe=True)
        for r, fr in ((0, 2), (1, 5)):
            bad = ~np.isfinite(got[r])
            assert bad[fr * hop:fr * hop + nh].all() and not bad[:fr * hop].any() and not bad[fr * hop + nh:].any(), (m, r)


# ---- both together -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [64, 240, 1024])
def test_round_trip_on_the_device(fft32, routes, oracle, m):
    """The two reconstructing pairs (the sine window at T = 1, and in block 1 of T = 3; D = M / 2) through the module's functions: the
    bytes of the oracle's round trip, which is x within the bound measured on the CPU (tests/test_pfb_cpu.py)."""
    from kofft_amd import pfb
    from test_pfb_cpu import ROUND_TRIP, rel

    hop = m // 2
    x = seeded(16100 + m).uniform(-1, 1, (3, 5 * m + 3)).astype(F)
    nx = x.shape[1]
    for taps in (1, 3):
        h = sine_pair(m, taps)
        lead = h.size - hop
        c, worst = pfb.reconstruction(h, h, m, hop)
        assert abs(c - 1.0) <= 1e-6 and worst <= 1e-6
        frames = -(-(nx + lead) // hop)
        Z = po.analysis_ref(x, h, m, hop, lead, frames, m // 2 + 1)
        want = np.ascontiguousarray(po.synthesis_ref(Z, h, m, hop, 1.0)[:, lead:lead + nx])
        assert rel(want, x) <= ROUND_TRIP[m]
        for f, _ in routes:
            spec = pfb.analysis(x, h, m, hop, lead=lead, fft=f)
            assert spec.shape == (3, frames, m // 2 + 1) and bits_equal(spec, Z)
            back = pfb.synthesis(spec, h, m, hop, out_first=lead, out_len=nx, fft=f)
            assert_rows_equal(back, want, f"pfb round trip M={m} T={taps}")
    one = pfb.synthesis(pfb.analysis(x[0], h, m, hop, lead=lead, fft=fft32), h, m, hop, out_first=lead, out_len=nx, fft=fft32)
    assert one.shape == (nx,) and bits_equal(one, want[0])


def test_shared_context_with_mdct_and_stft(fft32, oracle):
    """pfb, mdct and stft_rows calls alternating on one context (they share its tables and scratch) give unchanged results."""
    import mdct_oracle as mo
    from kofft_amd import mdct as km

    rng = seeded(16200)
    x = rng.uniform(-1, 1, (3, 3000)).astype(F)
    cases = []
    for m, taps, hop in ((256, 4, 256), (240, 2, 100)):
        h = rng.uniform(0.1, 1, taps * m).astype(F)
        frames = _covering(3000, 0, hop)
        Z = po.analysis_ref(x, h, m, hop, 0, frames, m // 2 + 1)
        cases.append((m, hop, h, frames, Z, po.synthesis_ref(Z, h, m, hop, 1.0)))
    w = km.sine_window(256)
    want_mdct = mo.mdct_ref(x, w, 256, 13)
    win = rng.uniform(0.1, 1, 240).astype(F)
    want_stft = oracle.stft_mt(x[0], win, 100, 30).reshape(30, 240)
    for _ in range(3):
        for m, hop, h, frames, Z, y in cases:
            assert bits_equal(fft32.pfb_analysis(x, h, m, hop, 0, frames, m // 2 + 1), Z)
            assert bits_equal(fft32.mdct_rows(x, w, 256, 13), want_mdct)
            assert bits_equal(fft32.pfb_synthesis(Z, h, m, hop), y)
            assert bits_equal(fft32.stft_rows(x[:1], win, 100, 30)[0], want_stft)


def test_python_errors(fft32):
    import kofft_amd

    E = kofft_amd.FftError
    x = np.ones((2, 100), F)
    h = np.ones(16, F)
    S = np.ones((2, 3, 5), np.complex64)
    for call, code in [(lambda: fft32.pfb_analysis(x, h, 7, 4, 0, 5, 3), E.InvalidValue), (lambda: fft32.pfb_analysis(x, h, 8, 4, 0, 5, 9), E.InvalidValue),
                       (lambda: fft32.pfb_analysis(x, h, 8, 0, 0, 5, 5), E.InvalidHopSize), (lambda: fft32.pfb_analysis(x, h, 8, 4, 16, 5, 5), E.InvalidValue),
                       (lambda: fft32.pfb_analysis(x, np.ones(0, F), 8, 4, 0, 5, 5), E.EmptyInput),
                       (lambda: fft32.pfb_synthesis(S, h, 16, 4), E.InvalidValue), (lambda: fft32.pfb_synthesis(S, h, 8, 0), E.InvalidHopSize),
                       (lambda: fft32.pfb_synthesis(S, h, 8, 4, first=20, count=5), E.MismatchedLengths)]:
        with pytest.raises(E) as e:
            call()
        assert e.value == E(code)
    with pytest.raises(E) as e:  # the switch takes 0, 1 and 2; a refused value leaves it as it was
        fft32.set_pfb_fused(3)
    assert e.value == E(E.InvalidValue)
    with pytest.raises(TypeError):
        fft32.pfb_analysis(x, np.ones((2, 8), F), 8, 4, 0, 5, 5)
    with pytest.raises(TypeError):
        fft32.pfb_synthesis(np.ones((2, 3, 5), F), h, 8, 4)
    assert fft32.pfb_analysis(x, h, 8, 4, 0, 0, 5).shape == (2, 0, 5)
    assert fft32.pfb_synthesis(S, h, 8, 4, count=0).shape == (2, 0)
    assert fft32.pfb_synthesis(np.ones((2, 0, 5), np.complex64), h, 8, 4).shape == (2, 0)
