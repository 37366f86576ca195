"""IIR filtering of rows by a cascade of biquads on the device, bit for bit against tests/sosfilt_oracle.py.  A default
context runs the kernel the measured rule names (kofft_hip_sosfilt_route: the tiled one from 16 rows on); a context with
set_sosfilt_tiled(0) runs the plain kernel always, one with set_sosfilt_tiled(2) the tiled kernel always.  Every call runs
twice and its two results are compared; the three contexts get the same inputs and must give the same bytes.  T (samples per tile) and G
(sections per pass) are read from the header."""
import re

import numpy as np
import pytest

from conftest import bits_equal, seeded
from rowcheck import assert_rows_equal
from sosfilt_oracle import cascade, designs, sosfilt_ref, sosfiltfilt_ref

pytestmark = pytest.mark.gpu
F = np.float32


def _define(name):
    from kofft_amd import _lib

    return int(re.search(rf"#define KOFFT_HIP_SOSFILT_{name} (\d+)", _lib.HEADER_PATH.read_text()).group(1))


T = _define("TILE")
G = _define("GROUP")


@pytest.fixture(scope="module")
def plain32():
    """A context with the tiled route off (set_sosfilt_tiled(0)): every call on the plain kernel."""
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    f.set_sosfilt_tiled(0)
    t = kofft_amd.HipFftImpl(F)
    t.set_sosfilt_tiled(2)  # the tiled kernel also below the rule's row count
    f.tiled = t
    yield f
    t.close()
    f.close()


def _rand(seed, rows, nx, sections, state=True):
    rng = seeded(seed)
    x = rng.uniform(-1, 1, (rows, nx)).astype(F)
    zi = rng.uniform(-1, 1, (rows, sections, 2)).astype(F) if state else None
    return x, zi


def _host(f, x, sos, zi, zf, reverse, off=0, inplace=False):
    res = []
    for _ in range(2):
        if inplace:
            buf = x.copy()
            st = None if zi is None else zi.copy()
            got = f.sosfilt_rows(buf, sos, zi=st, zf=zf, reverse=reverse, out=buf)
            if zf:
                assert got[0] is buf and (st is None or got[1] is st)
            else:
                assert got is buf
        else:
            got = f.sosfilt_rows(x, sos, zi=zi, zf=zf, reverse=reverse)
        res.append(got if zf else (got, None))
    assert bits_equal(res[0][0], res[1][0]) and (not zf or bits_equal(res[0][1], res[1][1])), "sosfilt_rows: two runs of the same call differ"
    return res[0]


def _dev(f, x, sos, zi, zf, reverse, off=0, inplace=False):
    """The device entry on torch buffers, twice; off: floats by which every buffer is shifted into its allocation; inplace: out == x
    and zf == zi."""
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
        f.sosfilt_dev(ptr(d_x), rows, nx, ptr(d_sos), sections, ptr(d_zi), ptr(d_zf), ptr(d_out), reverse=reverse)
        f.synchronize()
        if not inplace:
            assert bits_equal(d_x[off:].cpu().numpy(), x.reshape(-1)), "the input was modified"
            if d_zi is not None and d_zf is not d_zi:
                assert bits_equal(d_zi[off:].cpu().numpy(), zi.reshape(-1)), "the initial state was modified"
        assert bits_equal(d_sos[off:].cpu().numpy(), sos.reshape(-1))
        res.append((d_out[off:].cpu().numpy().reshape(rows, nx), None if d_zf is None else d_zf[off:].cpu().numpy().reshape(rows, sections, 2)))
    assert bits_equal(res[0][0], res[1][0]) and (not zf or bits_equal(res[0][1], res[1][1])), "sosfilt_dev: two runs of the same call differ"
    return res[0]


def _both(fft32, plain32, x, sos, zi, what, zf=True, reverse=False, want=None, nan_safe=False, run=_dev, off=0, inplace=False):
    """Both contexts against the oracle and against each other; returns the default context's (y, zf)."""
    if want is None:
        want = sosfilt_ref(sos, x, zi, reverse)
    out = []
    for f, route in ((fft32, "default route"), (plain32, "plain route"), (plain32.tiled, "tiled route")):
        y, z = run(f, x, sos, zi, zf, reverse, off, inplace)
        assert_rows_equal(y, want[0], f"{what}: {route}: outputs", nan_safe=nan_safe)
        if zf:
            assert_rows_equal(z.reshape(x.shape[0], -1), want[1].reshape(x.shape[0], -1), f"{what}: {route}: final states", nan_safe=nan_safe)
        else:
            assert z is None
        out.append((y, z))
    assert_rows_equal(out[0][0], out[1][0], what + ": the default and the plain route differ", nan_safe=nan_safe)
    assert_rows_equal(out[2][0], out[1][0], what + ": the tiled and the plain route differ", nan_safe=nan_safe)
    return out[0]


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("rows", [1, 2, 63, 64, 65, 255, 256, 257, 600])
def test_row_ladder(fft32, plain32, rows, reverse):
    nx = 2 * T + 5
    sos = cascade(2)
    x, zi = _rand(29400 + rows, rows, nx, 2)
    _both(fft32, plain32, x, sos, zi, f"rows={rows} nx={nx} reverse={reverse}", reverse=reverse)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("nx", [1, 2, 3, T - 1, T, T + 1, 2 * T, 2 * T + 1, 5 * T + 7])
def test_time_ladder(fft32, plain32, nx, reverse):
    sos = cascade(3)
    x, zi = _rand(29500 + nx, 67, nx, 3)
    _both(fft32, plain32, x, sos, zi, f"rows=67 nx={nx} reverse={reverse}", reverse=reverse)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("sections", [1, 2, G - 1, G, G + 1, 2 * G, 2 * G + 1])
def test_section_ladder(fft32, plain32, sections, reverse):
    nx = T + 3
    sos = cascade(sections)
    x, zi = _rand(29600 + sections, 65, nx, sections)
    want = sosfilt_ref(sos, x, zi, reverse)
    what = f"rows=65 nx={nx} sections={sections} reverse={reverse}"
    _both(fft32, plain32, x, sos, zi, what, reverse=reverse, want=want)
    _both(fft32, plain32, x, sos, zi, what + " host", reverse=reverse, want=want, run=_host)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("with_zi,with_zf", [(False, False), (False, True), (True, False), (True, True)])
def test_state_given_or_null(fft32, plain32, with_zi, with_zf, reverse):
    sections = G + 2
    sos = cascade(sections)
    x, zi = _rand(29700, 70, 2 * T + 3, sections, state=with_zi)
    want = sosfilt_ref(sos, x, zi, reverse)
    for run in (_dev, _host):
        _both(fft32, plain32, x, sos, zi, f"zi={with_zi} zf={with_zf} reverse={reverse} {run.__name__}", zf=with_zf, reverse=reverse, want=want, run=run)


@pytest.mark.parametrize("reverse", [False, True])
def test_a_row_in_two_calls_equals_one_call(fft32, plain32, reverse):
    """zf of the first call as zi of the second, the row cut at 1, T - 1, T, T + 1 and in the middle of a tile: the bits of one call.
    With the reverse flag the first call takes the end of the row."""
    sections, rows, nx = G + 1, 66, 3 * T + 11
    sos = cascade(sections)
    x, zi = _rand(29800, rows, nx, sections)
    whole_y, whole_z = sosfilt_ref(sos, x, zi, reverse)
    for cut in (1, T - 1, T, T + 1, T + T // 2, nx - 1):
        first, second = (x[:, nx - cut:], x[:, :nx - cut]) if reverse else (x[:, :cut], x[:, cut:])
        first, second = np.ascontiguousarray(first), np.ascontiguousarray(second)
        y1, z1 = _both(fft32, plain32, first, sos, zi, f"cut={cut} reverse={reverse}: first part", reverse=reverse)
        y2, z2 = _both(fft32, plain32, second, sos, z1, f"cut={cut} reverse={reverse}: second part", reverse=reverse)
        got = np.concatenate([y2, y1] if reverse else [y1, y2], axis=1)
        assert_rows_equal(got, whole_y, f"cut={cut} reverse={reverse}: two calls against one")
        assert_rows_equal(z2.reshape(rows, -1), whole_z.reshape(rows, -1), f"cut={cut} reverse={reverse}: final state")


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("sections", [3, 2 * G + 1])
def test_in_place(fft32, plain32, sections, reverse):
    """out == x and zf == zi, on both entry points."""
    sos = cascade(sections)
    x, zi = _rand(29900 + sections, 130, 2 * T + 9, sections)
    want = sosfilt_ref(sos, x, zi, reverse)
    for run in (_dev, _host):
        _both(fft32, plain32, x, sos, zi, f"in place sections={sections} reverse={reverse} {run.__name__}", reverse=reverse, want=want, run=run,
              inplace=True)
    _both(fft32, plain32, x, sos, None, f"in place, no state, sections={sections}", zf=False, reverse=reverse, run=_dev, inplace=True)


def test_grid_stride(fft32, plain32):
    """300 000 rows of 8 samples: more row groups (4688) and more rows than one launch of either kernel holds at once."""
    sos = cascade(1)
    x, zi = _rand(30000, 300000, 8, 1)
    _both(fft32, plain32, x, sos, zi, "300000 x 8")


def test_subnormal_decay_tail(fft32, plain32):
    """An impulse and 5999 zeros: the tail decays through the float32 subnormals, which the device keeps."""
    sos = designs()["butter4_low"]
    x = np.zeros((3, 6000), F)
    x[0, 0] = 1
    x[2, 5] = -1
    want = sosfilt_ref(sos, x)
    sub = (want[0] != 0) & (np.abs(want[0]) < np.finfo(F).tiny)
    assert sub[0].sum() > 100 and not sub[1].any()
    for reverse in (False, True):
        _both(fft32, plain32, x[:, ::-1].copy() if reverse else x, sos, None, f"decay tail reverse={reverse}", reverse=reverse)


def test_overflow_to_inf_and_nan(fft32, plain32):
    """A section with poles of radius 1.5: the output overflows to Inf, then Inf - Inf is NaN."""
    r, th = 1.5, 0.7
    sos = np.array([[1, 0.5, 0.25, 1, -2 * r * np.cos(th), r * r], [0.5, 0.1, 0.2, 1, -0.3, 0.2]], F)
    x, zi = _rand(30100, 66, 700, 2)
    want = sosfilt_ref(sos, x, zi)
    assert np.isinf(want[0]).any() and np.isnan(want[0]).any() and np.isfinite(want[0][:, :50]).all()
    _both(fft32, plain32, x, sos, zi, "overflow", want=want, nan_safe=True)
    _both(fft32, plain32, x, sos, zi, "overflow reverse", reverse=True, nan_safe=True)


@pytest.mark.parametrize("reverse", [False, True])
def test_row_isolation(fft32, plain32, reverse):
    """One NaN and one Inf in single rows of a 130-row batch: every other row keeps the clean run's bits (a leak through the LDS tile
    would reach a neighbouring row)."""
    sos = cascade(3)
    x, zi = _rand(30200, 130, 3 * T + 5, 3)
    clean_y, clean_z = _both(fft32, plain32, x, sos, zi, "isolation: clean", reverse=reverse)
    bad = x.copy()
    bad[64, T + 1] = np.nan
    bad[31, 2] = np.inf
    y, z = _both(fft32, plain32, bad, sos, zi, "isolation: NaN and Inf", reverse=reverse, nan_safe=True)
    others = np.ones(130, bool)
    others[[31, 64]] = False
    assert bits_equal(y[others], clean_y[others]) and bits_equal(z[others], clean_z[others]), "a special value reached another row"
    assert np.isnan(y[64]).any() and not np.isfinite(y[31]).all()
    _both(fft32, plain32, bad, sos, zi, "isolation host", reverse=reverse, nan_safe=True, run=_host)


@pytest.mark.parametrize("reverse", [False, True])
def test_unaligned_device_buffers(fft32, plain32, reverse):
    """Device buffers that are only 4-byte aligned (views one float into their allocations), rows of an odd length."""
    sos = cascade(2)
    x, zi = _rand(30300, 67, 2 * T + 5, 2)
    _both(fft32, plain32, x, sos, zi, f"unaligned reverse={reverse}", reverse=reverse, off=1)
    _both(fft32, plain32, x, sos, zi, f"unaligned in place reverse={reverse}", reverse=reverse, off=1, inplace=True)


@pytest.mark.parametrize("rows,nx", [(8, 10000), (64, 4000)])
def test_host_equals_device(fft32, plain32, rows, nx):
    """The host entry and the device entry give the same bytes: 320 KB in (below the 512 KiB zero-copy limit) and 1 MB (staged)."""
    sos = designs()["butter4_band"]
    x, zi = _rand(30400 + nx, rows, nx, sos.shape[0])
    want = sosfilt_ref(sos, x, zi)
    for f in (fft32, plain32, plain32.tiled):
        y, z = _host(f, x, sos, zi, True, False)
        assert_rows_equal(y, want[0], f"host rows={rows} nx={nx}")
        assert_rows_equal(z.reshape(rows, -1), want[1].reshape(rows, -1), f"host rows={rows} nx={nx}: states")
        yd, zd = _dev(f, x, sos, zi, True, False)
        assert bits_equal(y, yd) and bits_equal(z, zd), f"host against device rows={rows} nx={nx}"


def test_module_sosfilt(fft32, plain32):
    """kofft_amd.iir.sosfilt: scipy's state layout, 1-D and 2-D signals, bit for bit the oracle and scipy.signal.sosfilt on float32."""
    from scipy import signal

    from kofft_amd import iir

    sos = designs()["ellip8"]
    sections = sos.shape[0]
    x, zi = _rand(30500, 5, 900, sections)
    zi_scipy = np.ascontiguousarray(zi.transpose(1, 0, 2))
    want_y, want_z = sosfilt_ref(sos, x, zi)
    sy, sz = signal.sosfilt(sos, x, axis=-1, zi=zi_scipy)
    assert bits_equal(sy, want_y) and bits_equal(sz, want_z.transpose(1, 0, 2))
    for f in (fft32, plain32):
        y, zf = iir.sosfilt(sos, x, zi=zi_scipy, fft=f)
        assert_rows_equal(y, sy, "iir.sosfilt against scipy")
        assert zf.shape == (sections, 5, 2) and bits_equal(zf, sz)
        y0 = iir.sosfilt(sos, x, fft=f)
        assert_rows_equal(y0, sosfilt_ref(sos, x)[0], "iir.sosfilt without a state")
        one, z1 = iir.sosfilt(sos, x[0], zi=zi_scipy[:, 0], fft=f)
        assert one.shape == (900,) and z1.shape == (sections, 2) and bits_equal(one, sy[0]) and bits_equal(z1, sz[:, 0])
        r = iir.sosfilt(sos, x, reverse=True, fft=f)
        assert_rows_equal(r, signal.sosfilt(sos, x[:, ::-1], axis=-1)[:, ::-1], "iir.sosfilt reverse against scipy on the flipped rows")


@pytest.mark.parametrize("name", ["butter2_low", "butter4_high", "butter5_band", "butter6_low", "butter8_band", "ellip8"])
def test_module_sosfiltfilt(fft32, plain32, name):
    """kofft_amd.iir.sosfiltfilt: bit for bit the oracle's composition, and scipy.signal.sosfiltfilt in float64 under twice the margin
    measured on the CPU for the oracle on these data (tests/test_sosfilt_cpu.py)."""
    from scipy import signal

    from kofft_amd import iir
    from test_sosfilt_cpu import FILTFILT_MEASURED, _filtfilt_case

    sos, x = _filtfilt_case(name)
    want = sosfiltfilt_ref(sos, x)
    want64 = signal.sosfiltfilt(sos.astype(np.float64), x.astype(np.float64), axis=-1)
    for f in (fft32, plain32):
        got = iir.sosfiltfilt(sos, x, fft=f)
        assert_rows_equal(got, want, f"sosfiltfilt {name}")
        rel = float(np.max(np.abs(got.astype(np.float64) - want64)) / np.max(np.abs(want64)))
        print(f"{name}: max|d| / max|y| = {rel:.3e}")
        assert rel <= 2 * FILTFILT_MEASURED
        assert bits_equal(iir.sosfiltfilt(sos, x[0], fft=f), want[0])
        assert_rows_equal(iir.sosfiltfilt(sos, x, padlen=0, fft=f), sosfiltfilt_ref(sos, x, 0), f"sosfiltfilt {name} padlen=0")


def test_errors_that_need_a_context(fft32):
    import torch

    import kofft_amd

    E = kofft_amd.FftError
    x = np.ones((2, 10), F)
    sos = cascade(2)
    bad = sos.copy()
    bad[1, 3] = 2
    with pytest.raises(E) as e:
        fft32.sosfilt_rows(x, bad)
    assert e.value == E(E.InvalidValue)
    with pytest.raises(E) as e:
        fft32.sosfilt_rows(x, np.ones((0, 6), F))
    assert e.value == E(E.EmptyInput)
    with pytest.raises(E) as e:
        fft32.sosfilt_rows(x, sos, zi=np.ones((2, 3, 2), F))
    assert e.value == E(E.MismatchedLengths)
    for mode in (-1, 3):
        with pytest.raises(E) as e:
            fft32.set_sosfilt_tiled(mode)
        assert e.value == E(E.InvalidValue)
    assert fft32.sosfilt_rows(np.ones((0, 10), F), sos).shape == (0, 10) and fft32.sosfilt_rows(np.ones((2, 0), F), sos).shape == (2, 0)
    buf = torch.zeros(256, dtype=torch.float32, device="cuda")
    p = buf.data_ptr()
    with pytest.raises(kofft_amd.DeviceError):
        fft32.sosfilt_dev(0, 2, 10, p + 400, 2, 0, 0, p + 512)  # a null signal
    with pytest.raises(E) as e:
        fft32.sosfilt_dev(p, 2, 10, p + 400, 2, 0, 0, p + 512, flags=2)  # an unknown flag bit
    assert e.value == E(E.InvalidValue)
    # (d_x, d_sos, d_zi, d_zf, d_out): out over x, zf over zi, out over sos, zf over out, zf over x, out over zi
    for args in [(p, p + 400, 0, 0, p + 36), (p, p + 400, p + 600, p + 608, p + 100), (p, p + 100, 0, 0, p + 96),
                 (p, p + 400, 0, p + 120, p + 100), (p, p + 400, 0, p + 40, p + 100), (p, p + 400, p + 120, 0, p + 100)]:
        with pytest.raises(E) as e:
            fft32.sosfilt_dev(args[0], 2, 10, args[1], 2, args[2], args[3], args[4])
        assert e.value == E(E.InvalidValue), [a - p if a else 0 for a in args]
    fft32.synchronize()
    assert not buf.any()  # nothing ran


def test_route_modes_give_the_same_bytes():
    """set_sosfilt_tiled(2), the tiled kernel wherever it exists, against the oracle: the mode the measurements use."""
    import kofft_amd

    f = kofft_amd.HipFftImpl(F)
    try:
        f.set_sosfilt_tiled(2)
        sos = cascade(G + 3)
        x, zi = _rand(30600, 129, 4 * T + 1, G + 3)
        for reverse in (False, True):
            want = sosfilt_ref(sos, x, zi, reverse)
            y, z = _dev(f, x, sos, zi, True, reverse)
            assert_rows_equal(y, want[0], f"mode 2 reverse={reverse}")
            assert_rows_equal(z.reshape(129, -1), want[1].reshape(129, -1), f"mode 2 reverse={reverse}: states")
        f.set_sosfilt_tiled(1)
    finally:
        f.close()
