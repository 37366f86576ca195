"""IIR filtering of rows as a scan along time (kofft_hip_sosfilt_scan_f32) on the device, bit for bit against
tests/sosfilt_scan_oracle.py: forward and reverse, the host and the device entry point, every call twice on one context.  The chunks
are 32, 64 and 96 samples -- one, two and three tiles -- so that a few thousand samples cross many seams; a wavefront owns 64
(row, chunk) pairs, and the shapes put fewer than 64, exactly 64 and more than 64 chunks into a row and two and three rows into a wave."""
import re

import numpy as np
import pytest

from conftest import bits_equal, seeded
from rowcheck import assert_rows_equal
from sosfilt_oracle import cascade, designs, sosfilt_ref
from sosfilt_scan_oracle import sosfilt_scan_ref, sosfiltfilt_scan_ref

pytestmark = pytest.mark.gpu
F = np.float32
KNOB = "KOFFT_HIP_SCRATCH_CHUNK_MB"


def _define(name):
    from kofft_amd import _lib

    return int(re.search(rf"#define KOFFT_HIP_SOSFILT_{name} (\d+)", _lib.HEADER_PATH.read_text()).group(1))


T = _define("TILE")
G = _define("GROUP")
CHUNKS = [T, 2 * T, 3 * T]
NXS = [1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 43 * 32 - 7, 64 * 32 + 5, 130 * 32 + 1]


def _rand(seed, rows, nx, sections, state=True):
    rng = seeded(seed)
    x = rng.uniform(-1, 1, (rows, nx)).astype(F)
    zi = rng.uniform(-1, 1, (rows, sections, 2)).astype(F) if state else None
    return x, zi


def _host(f, x, sos, zi, zf, chunk, reverse, off=0, inplace=False):
    res = []
    for _ in range(2):
        if inplace:
            buf = x.copy()
            st = None if zi is None else zi.copy()
            got = f.sosfilt_scan_rows(buf, sos, chunk, zi=st, zf=zf, reverse=reverse, out=buf)
            if zf:
                assert got[0] is buf and (st is None or got[1] is st)
            else:
                assert got is buf
        else:
            got = f.sosfilt_scan_rows(x, sos, chunk, zi=zi, zf=zf, reverse=reverse)
        res.append(got if zf else (got, None))
    assert bits_equal(res[0][0], res[1][0]) and (not zf or bits_equal(res[0][1], res[1][1])), "sosfilt_scan_rows: two runs of the same call differ"
    return res[0]


def _dev(f, x, sos, zi, zf, chunk, reverse, off=0, inplace=False, call=None):
    """The device entry on torch buffers, twice; off: floats by which every buffer is shifted into its allocation; inplace: out == x
    and zf == zi; call: another device entry with sosfilt_dev's arguments (the sequential filter, for the single-chunk comparison)."""
    import torch

    rows, nx = x.shape
    sections = sos.shape[0]

    def up(a):
        t = torch.zeros(a.size + off, dtype=torch.float32, device="cuda")
        t[off:] = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
        return t

    d_sos = up(sos)
    res = []
    for _ in range(2):
        d_x = up(x)
        d_zi = None if zi is None else up(zi)
        d_out = d_x if inplace else torch.full((x.size + off,), float("nan"), dtype=torch.float32, device="cuda")
        if not zf:
            d_zf = None
        elif inplace and d_zi is not None:
            d_zf = d_zi
        else:
            d_zf = torch.full((rows * sections * 2 + off,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # (torch's copies and fills run on its stream, the call on the context's own)
        ptr = lambda t: 0 if t is None else t.data_ptr() + 4 * off  # noqa: E731
        if call is None:
            f.sosfilt_scan_dev(ptr(d_x), rows, nx, ptr(d_sos), sections, ptr(d_zi), ptr(d_zf), chunk, ptr(d_out), reverse=reverse)
        else:
            call(ptr(d_x), rows, nx, ptr(d_sos), sections, ptr(d_zi), ptr(d_zf), ptr(d_out), reverse=reverse)
        f.synchronize()
        if not inplace:
            assert bits_equal(d_x[off:].cpu().numpy(), x.reshape(-1)), "the input was modified"
            if d_zi is not None and d_zf is not d_zi:
                assert bits_equal(d_zi[off:].cpu().numpy(), zi.reshape(-1)), "the initial state was modified"
        assert bits_equal(d_sos[off:].cpu().numpy(), sos.reshape(-1))
        res.append((d_out[off:].cpu().numpy().reshape(rows, nx), None if d_zf is None else d_zf[off:].cpu().numpy().reshape(rows, sections, 2)))
    assert bits_equal(res[0][0], res[1][0]) and (not zf or bits_equal(res[0][1], res[1][1])), "sosfilt_scan_dev: two runs of the same call differ"
    return res[0]


def _check(f, x, sos, zi, chunk, what, zf=True, reverse=False, want=None, nan_safe=False, run=_dev, off=0, inplace=False):
    if want is None:
        want = sosfilt_scan_ref(sos, x, chunk, zi, reverse)
    y, z = run(f, x, sos, zi, zf, chunk, reverse, off, inplace)
    assert_rows_equal(y, want[0], f"{what}: outputs", nan_safe=nan_safe)
    if zf:
        assert_rows_equal(z.reshape(x.shape[0], -1), want[1].reshape(x.shape[0], -1), f"{what}: final states", nan_safe=nan_safe)
    else:
        assert z is None
    return y, z


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("chunk", CHUNKS)
def test_time_ladder(fft32, chunk, reverse):
    """Every length class of the short last chunk, rows of one chunk, of fewer than 64, of 64 and of more than 64 chunks; three rows,
    so a wavefront's 64 chunks span rows."""
    sos = cascade(2)
    for nx in NXS:
        x, zi = _rand(31000 + nx, 3, nx, 2)
        _check(fft32, x, sos, zi, chunk, f"rows=3 nx={nx} chunk={chunk} reverse={reverse}", reverse=reverse)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("rows", [1, 2, 3, 63, 64, 65])
def test_row_ladder(fft32, rows, reverse):
    """43 chunks a row (the last one short): three rows are 129 chunks, a wavefront's 64 span two and three rows."""
    nx, chunk = 43 * 32 - 7, 32
    sos = cascade(3)
    x, zi = _rand(31100 + rows, rows, nx, 3)
    _check(fft32, x, sos, zi, chunk, f"rows={rows} nx={nx} chunk={chunk} reverse={reverse}", reverse=reverse)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("sections", [1, 2, G - 1, G, G + 1, 2 * G, 2 * G + 1])
def test_section_ladder(fft32, sections, reverse):
    """One, two and three groups of sections: a longer cascade is a composition of scans."""
    nx, chunk = 70 * 64 + 9, 64
    sos = cascade(sections)
    x, zi = _rand(31200 + sections, 3, nx, sections)
    want = sosfilt_scan_ref(sos, x, chunk, zi, reverse)
    what = f"rows=3 nx={nx} sections={sections} chunk={chunk} reverse={reverse}"
    _check(fft32, x, sos, zi, chunk, what, reverse=reverse, want=want)
    _check(fft32, x, sos, zi, chunk, what + " host", reverse=reverse, want=want, run=_host)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("with_zi,with_zf", [(False, False), (False, True), (True, False), (True, True)])
def test_state_given_or_null(fft32, with_zi, with_zf, reverse):
    sections = G + 2
    sos = cascade(sections)
    x, zi = _rand(31300, 5, 9 * T + 3, sections, state=with_zi)
    want = sosfilt_scan_ref(sos, x, 2 * T, zi, reverse)
    for run in (_dev, _host):
        _check(fft32, x, sos, zi, 2 * T, f"zi={with_zi} zf={with_zf} reverse={reverse} {run.__name__}", zf=with_zf, reverse=reverse, want=want, run=run)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("sections", [3, 2 * G + 1])
def test_in_place(fft32, sections, reverse):
    """out == x and zf == zi, on both entry points: both walks read a tile before they write it, and chunks are disjoint."""
    sos = cascade(sections)
    x, zi = _rand(31400 + sections, 4, 70 * T + 9, sections)
    want = sosfilt_scan_ref(sos, x, T, zi, reverse)
    for run in (_dev, _host):
        _check(fft32, x, sos, zi, T, f"in place sections={sections} reverse={reverse} {run.__name__}", reverse=reverse, want=want, run=run, inplace=True)
    _check(fft32, x, sos, None, T, f"in place, no state, sections={sections}", zf=False, reverse=reverse, inplace=True)


def test_in_place_state_with_more_wavefronts_than_one_launch_holds(fft32):
    """zf == zi on 3 x 11.2 M samples in chunks of 32: 1 050 000 chunks are 16 407 wavefronts' work, more than the launch's 16 384
    workgroups, so the wavefront that stores a row's zf can retire before the one that walks the row's chunk 0 starts.  The storing walk
    takes Z_0 from the scratch, not from zi: in place gives the bits of out of place (device against device; the oracle's carry over
    350 000 seams would take longer than the rest of this file)."""
    rows, nx, chunk = 3, 350000 * 32 + 5, 32
    sos = cascade(1)
    x, zi = _rand(32050, rows, nx, 1)
    y, z = _dev(fft32, x, sos, zi, True, chunk, False)
    yi, zi_after = _dev(fft32, x, sos, zi, True, chunk, False, inplace=True)
    assert bits_equal(y, yi), "in place: the outputs differ from out of place"
    assert bits_equal(z, zi_after), "in place: the final states differ from out of place"
    head, _ = _dev(fft32, np.ascontiguousarray(x[:, :chunk]), sos, zi, True, 0, False, call=fft32.sosfilt_dev)
    assert bits_equal(y[:, :chunk], head), "chunk 0 is the sequential filter's from zi"


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("off", [1, 3])
def test_unaligned_device_buffers(fft32, off, reverse):
    """Device buffers 4 and 12 bytes into their allocations, rows of an odd length."""
    sos = cascade(2)
    x, zi = _rand(31500, 3, 66 * T + 5, 2)
    want = sosfilt_scan_ref(sos, x, T, zi, reverse)
    _check(fft32, x, sos, zi, T, f"offset {4 * off} reverse={reverse}", reverse=reverse, want=want, off=off)
    _check(fft32, x, sos, zi, T, f"offset {4 * off} in place reverse={reverse}", reverse=reverse, want=want, off=off, inplace=True)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("chunk_tiles", [3, 4, 1 << 20])
def test_one_chunk_is_sosfilt(fft32, chunk_tiles, reverse):
    """chunk >= nx: the bytes of kofft_hip_dev_sosfilt_f32, device against device (nx = 3 T - 5: chunks of exactly ceil(nx / T) tiles,
    of one more, and of 2^25 samples)."""
    sections = G + 1
    sos = cascade(sections)
    x, zi = _rand(31600, 67, 3 * T - 5, sections)
    y, z = _dev(fft32, x, sos, zi, True, chunk_tiles * T, reverse)
    ys, zs = _dev(fft32, x, sos, zi, True, 0, reverse, call=fft32.sosfilt_dev)
    assert_rows_equal(y, ys, "one chunk against sosfilt")
    assert_rows_equal(z.reshape(67, -1), zs.reshape(67, -1), "one chunk against sosfilt: states")
    assert_rows_equal(ys, sosfilt_ref(sos, x, zi, reverse)[0], "sosfilt against its oracle")


@pytest.mark.parametrize("reverse", [False, True])
def test_first_chunk_is_sosfilt(fft32, reverse):
    """Chunk 0 of any call equals the sequential filter's first `chunk` samples (the last ones in time with the reverse flag)."""
    sos = cascade(4)
    x, zi = _rand(31700, 3, 10 * T + 3, 4)
    y, _ = _check(fft32, x, sos, zi, 2 * T, f"first chunk reverse={reverse}", reverse=reverse)
    ys, _ = _dev(fft32, x, sos, zi, True, 0, reverse, call=fft32.sosfilt_dev)
    first = np.s_[:, -2 * T:] if reverse else np.s_[:, :2 * T]
    assert bits_equal(y[first], ys[first])


@pytest.mark.parametrize("reverse", [False, True])
def test_row_isolation(fft32, reverse):
    """A NaN sample in one row and an Inf sample in another: every other row keeps the clean run's bits (a leak through the LDS tile,
    the state scratch or a wavefront shared by two rows would reach a neighbour)."""
    sos = cascade(3)
    rows, nx, chunk = 5, 43 * 32 - 7, 32
    x, zi = _rand(31800, rows, nx, 3)
    clean_y, clean_z = _check(fft32, x, sos, zi, chunk, "isolation: clean", reverse=reverse)
    bad = x.copy()
    bad[1, 40 * 32 + 1] = np.nan
    bad[3, 2] = np.inf
    y, z = _check(fft32, bad, sos, zi, chunk, "isolation: NaN and Inf", reverse=reverse, nan_safe=True)
    others = np.array([True, False, True, False, True])
    assert bits_equal(y[others], clean_y[others]) and bits_equal(z[others], clean_z[others]), "a special value reached another row"
    assert np.isnan(y[1]).any() and not np.isfinite(y[3]).all()
    _check(fft32, bad, sos, zi, chunk, "isolation host", reverse=reverse, nan_safe=True, run=_host)


def test_inf_in_a_late_sections_state(fft32):
    """zi = Inf in the last section of a group: the carry's triangular sum leaves the earlier sections' zf finite (a full row of M times
    the state would multiply the Inf by M's exact zeros)."""
    sections = 4
    sos = cascade(sections)
    x, zi = _rand(31900, 2, 9 * T + 1, sections)
    zi[0, 3, 0] = np.inf
    want = sosfilt_scan_ref(sos, x, T, zi)
    assert np.isfinite(want[1][:, :3]).all() and not np.isfinite(want[1][0, 3]).all() and np.isfinite(want[1][1]).all()
    for run in (_dev, _host):
        _check(fft32, x, sos, zi, T, f"Inf in zi {run.__name__}", want=want, nan_safe=True, run=run)


def test_subnormal_decay_tail(fft32):
    """An impulse and 5999 zeros in chunks of 96: the tail decays through the float32 subnormals across the seams; the carry keeps them."""
    sos = designs()["butter4_low"]
    x = np.zeros((3, 6000), F)
    x[0, 0] = 1
    x[2, 5] = -1
    want = sosfilt_scan_ref(sos, x, 3 * T)
    sub = (want[0] != 0) & (np.abs(want[0]) < np.finfo(F).tiny)
    assert sub[0].sum() > 50 and not sub[1].any(), "the expected output holds subnormals (62 seams cross the tail)"
    for reverse in (False, True):
        _check(fft32, x[:, ::-1].copy() if reverse else x, sos, None, 3 * T, f"decay tail reverse={reverse}", reverse=reverse)


def test_states_beyond_the_scratch_cap(monkeypatch):
    """KOFFT_HIP_SCRATCH_CHUNK_MB=1 around a context of the test's own: 8 sections in chunks of 32 keep 64 bytes a seam, 3750 seams and
    the copy of Z_0 of a row of 120 001 samples are 240 064 bytes, four rows a piece: five rows go as 4 + 1, and the second piece starts
    at row 4."""
    import kofft_amd

    rows, nx, chunk = 5, 120001, 32
    assert (1 << 20) // (((nx - 1) // chunk + 1) * 16 * 4) == 4
    sos = cascade(G)
    x, zi = _rand(32000, rows, nx, G)
    want = sosfilt_scan_ref(sos, x, chunk, zi)
    monkeypatch.setenv(KNOB, "1")
    f = kofft_amd.HipFftImpl(F)
    try:
        _check(f, x, sos, zi, chunk, "pieces of rows", want=want)
        _check(f, x, sos, zi, chunk, "pieces of rows, host", want=want, run=_host)
    finally:
        f.close()


def test_module_functions(fft32):
    """kofft_amd.iir.sosfilt_scan: scipy's state layout, 1-D and 2-D signals, the default chunk, and the float64 scipy bound of the CPU
    test (tests/test_sosfilt_scan_cpu.py: twice the measured error of the oracle on these data)."""
    from scipy import signal

    from kofft_amd import iir
    from test_sosfilt_scan_cpu import ACCURACY_MEASURED, FILTFILT_SCAN_MEASURED, GPU_CASES, _accuracy_case, _filtfilt_case, rel_err

    sos = designs()["ellip8"]
    sections = sos.shape[0]
    x, zi = _rand(32100, 5, 900, sections)
    zi_scipy = np.ascontiguousarray(zi.transpose(1, 0, 2))
    want_y, want_z = sosfilt_scan_ref(sos, x, 64, zi)
    y, zf = iir.sosfilt_scan(sos, x, zi=zi_scipy, chunk=64, fft=fft32)
    assert_rows_equal(y, want_y, "iir.sosfilt_scan")
    assert zf.shape == (sections, 5, 2) and bits_equal(zf, want_z.transpose(1, 0, 2))
    one, z1 = iir.sosfilt_scan(sos, x[0], zi=zi_scipy[:, 0], chunk=64, fft=fft32)
    assert one.shape == (900,) and z1.shape == (sections, 2) and bits_equal(one, want_y[0]) and bits_equal(z1, want_z[0])
    r = iir.sosfilt_scan(sos, x, chunk=64, reverse=True, fft=fft32)
    assert_rows_equal(r, sosfilt_scan_ref(sos, x, 64, reverse=True)[0], "iir.sosfilt_scan reverse")
    k = iir.scan_chunk(5, 900, sections)
    assert k >= 1024 and k % T == 0
    assert_rows_equal(iir.sosfilt_scan(sos, x, fft=fft32), sosfilt_ref(sos, x)[0], "the default chunk holds the whole row: sosfilt's bytes")
    for name, chunk in GPU_CASES:
        measured = ACCURACY_MEASURED[name, chunk]
        dsos, dx, want64 = _accuracy_case(name, chunk)
        got = iir.sosfilt_scan(dsos, dx, chunk=chunk, fft=fft32)
        assert_rows_equal(got, sosfilt_scan_ref(dsos, dx, chunk)[0], f"{name} chunk={chunk}")
        e = rel_err(got, want64)
        print(f"{name} chunk={chunk}: E_scan = {e:.3e}")
        assert e <= 2 * measured
    for name in ("butter4_low", "ellip8"):
        fsos, fx = _filtfilt_case(name)
        got = iir.sosfiltfilt(fsos, fx, chunk=64, fft=fft32)
        assert_rows_equal(got, sosfiltfilt_scan_ref(fsos, fx, 64), f"sosfiltfilt chunk=64 {name}")
        e = rel_err(got, signal.sosfiltfilt(fsos.astype(np.float64), fx.astype(np.float64), axis=-1))
        print(f"sosfiltfilt {name} chunk=64: {e:.3e}")
        assert e <= 2 * FILTFILT_SCAN_MEASURED


def test_errors_that_need_a_context(fft32):
    import torch

    import kofft_amd

    E = kofft_amd.FftError
    x = np.ones((2, 100), F)
    sos = cascade(2)
    for chunk in (0, 33, T - 1):
        with pytest.raises(E) as e:
            fft32.sosfilt_scan_rows(x, sos, chunk)
        assert e.value == E(E.InvalidValue)
    bad = sos.copy()
    bad[1, 3] = 2
    with pytest.raises(E) as e:
        fft32.sosfilt_scan_rows(x, bad, T)
    assert e.value == E(E.InvalidValue)
    with pytest.raises(E) as e:
        fft32.sosfilt_scan_rows(x, np.ones((0, 6), F), T)
    assert e.value == E(E.EmptyInput)
    with pytest.raises(E) as e:
        fft32.sosfilt_scan_rows(x, sos, T, zi=np.ones((2, 3, 2), F))
    assert e.value == E(E.MismatchedLengths)
    assert fft32.sosfilt_scan_rows(np.ones((0, 10), F), sos, T).shape == (0, 10) and fft32.sosfilt_scan_rows(np.ones((2, 0), F), sos, 0).shape == (2, 0)
    buf = torch.zeros(256, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    with pytest.raises(kofft_amd.DeviceError):
        fft32.sosfilt_scan_dev(0, 2, 10, p + 400, 2, 0, 0, T, p + 512)  # a null signal
    with pytest.raises(E) as e:
        fft32.sosfilt_scan_dev(p, 2, 10, p + 400, 2, 0, 0, T, p + 512, flags=2)  # an unknown flag bit
    assert e.value == E(E.InvalidValue)
    with pytest.raises(E) as e:
        fft32.sosfilt_scan_dev(p, 2, 10, p + 400, 2, 0, 0, 48, p + 512)  # no multiple of the tile
    assert e.value == E(E.InvalidValue)
    with pytest.raises(E) as e:
        fft32.sosfilt_scan_dev(p, 2, 10, p + 400, 2, 0, 0, T, p + 36)  # out over x
    assert e.value == E(E.InvalidValue)
    fft32.synchronize()
    assert not buf.any()  # nothing ran
