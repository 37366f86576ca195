"""Seeded differential fuzz over the filter and lapped families: resample, sosfilt, sosfilt_scan, convolve_bank, the
fast DCT-IV, mdct and imdct on TWO contexts shared by every case of the module -- the default one and one created under
KOFFT_HIP_SCRATCH_CHUNK_MB=1 -- whose route switches change from case to case, so that table cache, grow-only scratch (real_tmp,
rows_tmp) and routes are whatever the calls before left behind.

tests/filter_cases.py draws the cases (one call each) and derives every expected value from the family's existing oracle.  Every row
of every output -- the final states of the two filters included -- is compared bit for bit (NaN-safe); every call runs twice on buffers
inside a guard-band arena (tests/redzone.py; the host form on a host arena): the same bytes twice, inputs and NaN gaps unchanged (an
in-place buffer excepted), nothing written outside an output.  The call a seed's draw has the header refuse returns its code and leaves
the prefilled outputs alone; the next case runs as usual.  Once per seed the scratch is released between two cases, and one case runs
on a side stream.  Finite cases are held to float64 within the bounds of the families' CPU tests (tests/test_filter_cases_cpu.py says
which, and holds the oracles to them).  A failure names seed, case, family, route, form and the whole geometry."""
import numpy as np
import pytest

import filter_cases as fc
from redzone import Arena
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32
KNOB = "KOFFT_HIP_SCRATCH_CHUNK_MB"


def _defaults(f):
    f.set_resample_tiled(1)
    f.set_sosfilt_tiled(1)
    f.set_convolve_bank_fused(True)
    f.set_mdct_fused(True)


def _route(f, case):
    if case.family == "resample":
        f.set_resample_tiled(case.route)
    elif case.family == "sosfilt":
        f.set_sosfilt_tiled(case.route)
    elif case.family == "convolve_bank":
        f.set_convolve_bank_fused(bool(case.route))
    elif case.family in ("dct4", "mdct", "imdct"):
        f.set_mdct_fused(bool(case.route))


@pytest.fixture(scope="module")
def contexts():
    """The two contexts of the module; the knob is read when a context is created and is put back right after."""
    import kofft_amd

    default = kofft_amd.HipFftImpl(F)
    mp = pytest.MonkeyPatch()
    mp.setenv(KNOB, "1")
    try:
        chunk1 = kofft_amd.HipFftImpl(F)
    finally:
        mp.undo()
    both = {"default": default, "chunk1": chunk1}
    yield both
    for f in both.values():
        _defaults(f)
        f.close()


@pytest.fixture(scope="module")
def helpers(hiplib):
    return fc.Helpers.from_lib(hiplib)


@pytest.fixture(scope="module")
def bounds():
    from test_filter_cases_cpu import float64_bounds

    return float64_bounds()


class Call:
    """One call on buffers of a guard-band arena: regions first, then run(): twice, the same bytes, the bands intact."""

    def __init__(self, f, case):
        self.f, self.what = f, case.describe()
        self.host = case.form == "host"
        self.arena = Arena("host" if self.host else "cuda", self.what)
        off = case.form in ("dev_off", "dev_unaligned")
        self.off4 = 4 if off else 0   # every f32 pointer 4 bytes off a 16-byte boundary
        self.off8 = 8 if off else 0   # complex outputs stay 8-byte aligned
        self.offx = 6 if case.form == "dev_unaligned" else self.off4  # the main input two more bytes off: not 4-byte aligned
        self.fn = getattr(f._lib, ("kofft_hip_" if self.host else "kofft_hip_dev_") + fc.ENTRY[case.family])
        self.outs = []

    def input(self, a, name, row_bytes=None, off=None):
        return self.arena.input(a, self.off4 if off is None else off, row_bytes, name)

    def output(self, nbytes, name, off=None, row_bytes=None):
        r = self.arena.output(nbytes, self.off4 if off is None else off, None, row_bytes, name)
        self.outs.append(r)
        return r

    def inout(self, a, name, row_bytes=None):
        r = self.arena.inout(a, self.off4, row_bytes, name)
        self.outs.append(r)
        return r

    def _read(self):
        self.f.synchronize()
        return {r.name: self.arena.read(r, np.uint8, (r.nbytes,)) for r in self.outs}

    def run(self, invoke, refused=None, stream=None):
        """invoke() -> the return code.  Returns the outputs' bytes by name (None for a refused call)."""
        for r in self.arena.regions:
            r.addr  # (lays the arena out before the first call)
        if stream is not None:
            self.f.set_stream(stream.cuda_stream)
        try:
            rc = invoke()
            first = self._read()
            if refused is not None:
                assert rc == refused, f"{self.what}: returned {rc}, the header says {refused}"
                for r in self.outs:
                    assert first[r.name].tobytes() == self.arena._host(r.start, r.start + r.nbytes, pristine=True).tobytes(), \
                        f"{self.what}: a refused call wrote to '{r.name}'"
                self.arena.verify()
                return None
            assert rc == 0, f"{self.what}: returned {rc}"
            for r in self.outs:
                self.arena.restore(r)
            rc = invoke()
            assert rc == 0, f"{self.what}: the second run returned {rc}"
            second = self._read()
        finally:
            if stream is not None:
                self.f.synchronize()
                self.f.set_stream(0)
        for r in self.outs:
            assert first[r.name].tobytes() == second[r.name].tobytes(), f"{self.what}: two runs of the same call differ in '{r.name}'"
        self.arena.verify()
        return first


def _regions(c, case, inp):
    """The call's buffers in the arena: (pointers by name, name -> (region name, dtype, shape) of every output)."""
    g, fam = case.g, case.family
    p, outs = {}, {}
    inplace = case.form == "inplace"
    if fam == "resample":
        p["x"] = c.input(inp["x"], "x", 4 * g["nx"])
        p["h"] = c.input(inp["h"], "h")
        p["out"] = c.output(g["rows"] * g["out_len"] * 4, "out", row_bytes=4 * g["out_len"])
        outs["out"] = (F, (g["rows"], g["out_len"]))
    elif fam in ("sosfilt", "sosfilt_scan"):
        rows, nx, sections = g["rows"], g["nx"], g["sections"]
        p["sos"] = c.input(inp["sos"], "sos")
        if inplace:
            p["x"] = p["out"] = c.inout(inp["x"], "out", 4 * nx)
        else:
            p["x"] = c.input(inp["x"], "x", 4 * nx)
            p["out"] = c.output(rows * nx * 4, "out", row_bytes=4 * nx)
        outs["out"] = (F, (rows, nx))
        if inplace and g["zi"] and g["zf"]:
            p["zi"] = p["zf"] = c.inout(inp["zi"], "zf", 8 * sections)
        else:
            if g["zi"]:
                p["zi"] = c.input(inp["zi"], "zi", 8 * sections)
            if g["zf"]:
                p["zf"] = c.output(rows * sections * 8, "zf", row_bytes=8 * sections)
        if g["zf"]:
            outs["zf"] = (F, (rows, sections, 2))
    elif fam == "convolve_bank":
        p["x"] = c.input(inp["x"], "x", 4 * g["nx"], off=c.offx)
        p["h"] = c.input(inp["h"], "h", inp["h"].itemsize * g["nh"])
        cplx = g["kind"] == "complex"
        el = 8 if cplx else 4
        p["out"] = c.output(g["rows"] * g["filters"] * g["out_len"] * el, "out", off=c.off8 if cplx else c.off4, row_bytes=el * g["out_len"])
        outs["out"] = (np.complex64 if cplx else F, (g["rows"], g["filters"], g["out_len"]))
    elif fam == "dct4":
        n, rows = g["n"], g["rows"]
        if inplace:
            p["x"] = p["out"] = c.inout(inp["x"], "out", 4 * n)
        else:
            p["x"] = c.input(inp["x"], "x", 4 * n, off=c.offx)
            p["out"] = c.output(rows * n * 4, "out", row_bytes=4 * n)
        outs["out"] = (F, (rows, n))
    elif fam == "mdct":
        p["x"] = c.input(fc.strided(inp["x"], g["row_stride"]), "x", 4 * g["row_stride"], off=c.offx)
        p["window"] = c.input(inp["window"], "window")
        p["out"] = c.output(g["rows"] * g["frames"] * g["n"] * 4, "out", row_bytes=4 * g["n"])
        outs["out"] = (F, (g["rows"], g["frames"], g["n"]))
    else:
        p["x"] = c.input(inp["x"], "coef", 4 * g["n"], off=c.offx)
        p["window"] = c.input(inp["window"], "window")
        p["out"] = c.output(g["rows"] * g["out_len"] * 4, "out", row_bytes=4 * g["out_len"])
        outs["out"] = (F, (g["rows"], g["out_len"]))
    return p, outs


def _case(f, case, bounds):
    import torch

    _route(f, case)
    if case.release_before:
        f.release_scratch()
    inp = fc.inputs(case)
    c = Call(f, case)
    regions, outs = _regions(c, case, inp)
    addr = {k: r.addr for k, r in regions.items()}
    stream = torch.cuda.Stream() if case.side_stream else None  # (a host form stages through that stream)
    got = c.run(lambda: fc.invoke(c.fn, f._ctx, case, addr), case.refuse["code"] if case.refuse else None, stream)
    if got is None:
        return
    want = fc.expected(case, inp)
    assert set(want) == set(outs), (case.describe(), sorted(want), sorted(outs))
    res = {}
    for name, (dtype, shape) in outs.items():
        res[name] = got[regions[name].name].view(dtype).reshape(shape)
        rows = shape[0] * (shape[1] if len(shape) == 3 and name == "out" else 1)
        assert_rows_equal(res[name].reshape(rows, -1), want[name].reshape(rows, -1), f"{case.describe()} output '{name}'", nan_safe=True)
    if not case.specials:
        held = fc.float64_error(case, inp, res, bounds)
        if held is not None:
            err, bound = held
            assert err <= bound, f"{case.describe()}: float64 error {err:.3g} > {bound:.3g}"


@pytest.mark.parametrize("seed", range(fc.SEEDS))
def test_fuzz_filters(contexts, helpers, bounds, oracle, seed):
    try:
        for case in fc.cases(seed, helpers):
            _case(contexts[case.ctx], case, bounds)
    finally:
        for f in contexts.values():
            _defaults(f)
