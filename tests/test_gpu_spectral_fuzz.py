"""Seeded differential fuzz over the spectral families: planar fft_split / ifft_split (f32 and f64), chirp-Z,
Goertzel, the Hartley transform and the polyphase filter bank, analysis and synthesis, on contexts shared by every case of the module
-- per precision the default one and one created under KOFFT_HIP_SCRATCH_CHUNK_MB=1 (only split uses the f64 pair) -- whose route
switches change from case to case, so that table cache, grow-only scratch (real_tmp, rows_tmp), the chirp-Z table slots, the
Goertzel coefficient set, the Hartley tables and the routes are whatever the calls before left behind.

tests/spectral_cases.py draws the cases (one call each) and derives every expected value from the family's existing oracle.  Every
row of every output is compared bit for bit (NaN-safe where the data or the chirp-Z parameters leave the finite range); every call runs
twice on buffers inside a guard-band arena (tests/redzone.py; the host form on a host arena): the same bytes twice, inputs and NaN gaps
unchanged (an in-place buffer excepted), nothing written outside an output.  The call a seed's draw has the header refuse returns its
code and leaves the prefilled outputs alone; the next case runs as usual.  Once per seed the scratch is released between two cases, and
one case runs on a side stream.  Finite chirp-Z and filter-bank cases are held to float64 within the bounds of the families' CPU tests
(tests/test_spectral_cases_cpu.py says which, and holds the oracles to them).  A failure names seed, case, family, route, form and the
whole geometry."""
import numpy as np
import pytest

import spectral_cases as sc
from redzone import Arena
from rowcheck import assert_rows_equal

pytestmark = pytest.mark.gpu
F = np.float32
KNOB = "KOFFT_HIP_SCRATCH_CHUNK_MB"


def _defaults(f):
    f.set_split_fused(True)
    if f.dtype == np.float32:
        f.set_czt_route(0)
        f.set_direct_tiled(True)
        f.set_dht_table_device(True)
        f.set_pfb_fused(1)


def _route(f, case):
    fam = case.family
    if fam in ("split32", "split64"):
        f.set_split_fused(bool(case.route))
    elif fam == "czt":
        f.set_czt_route(case.route)
        f.set_direct_tiled(bool(case.g["direct_tiled"]))
    elif fam == "dht":
        f.set_direct_tiled(bool(case.route))
        f.set_dht_table_device(bool(case.g["table_device"]))
    elif fam in ("pfb_analysis", "pfb_synthesis"):
        f.set_pfb_fused(case.route)


@pytest.fixture(scope="module")
def contexts():
    """(precision, "default" / "chunk1") -> context; the knob is read when a context is created and is put back right after."""
    import kofft_amd

    both = {}
    for real in (np.float32, np.float64):
        both[np.dtype(real).name, "default"] = kofft_amd.HipFftImpl(real)
        mp = pytest.MonkeyPatch()
        mp.setenv(KNOB, "1")
        try:
            both[np.dtype(real).name, "chunk1"] = kofft_amd.HipFftImpl(real)
        finally:
            mp.undo()
    yield both
    for f in both.values():
        _defaults(f)
        f.close()


@pytest.fixture(scope="module")
def bounds():
    from test_spectral_cases_cpu import float64_bounds

    return float64_bounds()


class Call:
    """One call on buffers of a guard-band arena: regions first, then run(): twice, the same bytes, the bands intact."""

    def __init__(self, f, case):
        self.f, self.what = f, case.describe()
        self.host = not case.device_form
        self.arena = Arena("host" if self.host else "cuda", self.what)
        off = case.form in ("dev_off", "dev_unaligned")
        self.off = np.dtype(case.real).itemsize if off else 0   # every real pointer one element off a 16-byte boundary
        self.off8 = 8 if off else 0                              # the complex pfb frames stay 8-byte aligned
        self.offx = 6 if case.form == "dev_unaligned" else self.off  # the analysis input two more bytes off: not 4-byte aligned
        self.fn = getattr(f._lib, ("kofft_hip_" if self.host else "kofft_hip_dev_") + sc.ENTRY[case.family])
        self.outs = []

    def input(self, a, name, row_bytes=None, off=None):
        return self.arena.input(a, self.off if off is None else off, row_bytes, name)

    def output(self, nbytes, name, off=None, row_bytes=None):
        r = self.arena.output(nbytes, self.off if off is None else off, None, row_bytes, name)
        self.outs.append(r)
        return r

    def inout(self, a, name, row_bytes=None):
        r = self.arena.inout(a, self.off, row_bytes, name)
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
    """The call's buffers in the arena: (pointers by name, name -> (region, dtype, shape) of every output)."""
    g, fam = case.g, case.family
    p, outs = {}, {}
    if fam in ("split32", "split64"):
        n, batch, el = g["n"], g["batch"], np.dtype(case.real).itemsize
        if case.form in ("host", "inplace"):
            p["re"] = p["re_out"] = c.inout(inp["re"], "re", el * n)
            p["im"] = p["im_out"] = c.inout(inp["im"], "im", el * n)
        else:
            p["re"], p["im"] = c.input(inp["re"], "re_in", el * n), c.input(inp["im"], "im_in", el * n)
            p["re_out"], p["im_out"] = c.output(batch * n * el, "re", row_bytes=el * n), c.output(batch * n * el, "im", row_bytes=el * n)
        outs["re"], outs["im"] = (p["re_out"], case.real, (batch, n)), (p["im_out"], case.real, (batch, n))
    elif fam == "czt":
        p["x"] = c.input(inp["x"], "x", 4 * g["n"])
        p["out"] = c.output(g["batch"] * g["m"] * 8, "out", row_bytes=8 * g["m"])
        outs["out"] = (p["out"], np.complex64, (g["batch"], g["m"]))
    elif fam == "goertzel":
        p["x"] = c.input(inp["x"], "x", 4 * g["n"])
        p["out"] = c.output(g["batch"] * g["nfreq"] * 4, "out", row_bytes=4 * g["nfreq"])
        outs["out"] = (p["out"], F, (g["batch"], g["nfreq"]))
    elif fam == "dht":
        if case.form == "inplace":
            p["x"] = p["out"] = c.inout(inp["x"], "out", 4 * g["n"])
        else:
            p["x"] = c.input(inp["x"], "x", 4 * g["n"])
            p["out"] = c.output(g["batch"] * g["n"] * 4, "out", row_bytes=4 * g["n"])
        outs["out"] = (p["out"], F, (g["batch"], g["n"]))
    elif fam == "pfb_analysis":
        p["x"] = c.input(sc.strided(inp["x"], g["row_stride"]), "x", 4 * g["row_stride"], off=c.offx)
        p["h"] = c.input(inp["h"], "h")
        p["out"] = c.output(g["rows"] * g["frames"] * g["bins"] * 8, "out", off=c.off8, row_bytes=8 * g["bins"])
        outs["out"] = (p["out"], np.complex64, (g["rows"], g["frames"], g["bins"]))
    else:
        p["x"] = c.input(inp["x"], "spec", 8 * g["bins"], off=c.off8)
        p["h"] = c.input(inp["h"], "g")
        p["out"] = c.output(g["rows"] * g["out_len"] * 4, "out", row_bytes=4 * g["out_len"])
        outs["out"] = (p["out"], F, (g["rows"], g["out_len"]))
    return p, outs


def _case(f, case, bounds):
    import ctypes as C

    import torch

    if case.release_before:
        f.release_scratch()
    if case.refuse and case.refuse.get("setter"):  # no call of the family: the setter refuses the value and keeps the route
        name, value = case.refuse["setter"]
        assert getattr(f._lib, name)(f._ctx, value) == case.refuse["code"], case.describe()
        return
    _route(f, case)
    inp = sc.inputs(case)
    c = Call(f, case)
    regions, outs = _regions(c, case, inp)
    addr = {k: r.addr for k, r in regions.items()}
    if case.family == "goertzel":
        freqs = np.ascontiguousarray(inp["freqs"], F)  # a host pointer in both forms
        addr["freqs"] = C.c_void_p(freqs.ctypes.data)
    if case.refuse and case.refuse.get("overlap"):
        addr["out"] = addr["x"]
    stream = torch.cuda.Stream() if case.side_stream else None  # (a host form stages through that stream)
    got = c.run(lambda: sc.invoke(c.fn, f._ctx, case, addr, c.host), case.refuse["code"] if case.refuse else None, stream)
    if got is None:
        return
    want = sc.expected(case, inp)
    assert set(want) == set(outs), (case.describe(), sorted(want), sorted(outs))
    res = {}
    for name, (region, dtype, shape) in outs.items():
        res[name] = got[region.name].view(dtype).reshape(shape)
        rows = shape[0] * (shape[1] if len(shape) == 3 else 1)
        if res[name].size:
            assert_rows_equal(res[name].reshape(rows, -1), want[name].reshape(rows, -1), f"{case.describe()} output '{name}'", nan_safe=sc.nan_safe(case))
    if not case.specials:
        held = sc.float64_error(case, inp, res, bounds)
        if held is not None:
            err, bound = held
            assert err <= bound, f"{case.describe()}: float64 error {err:.3g} > {bound:.3g}"


@pytest.mark.parametrize("seed", range(sc.SEEDS))
def test_fuzz_spectral(contexts, bounds, oracle, seed):
    try:
        for case in sc.cases(seed):
            _case(contexts[np.dtype(case.real).name, case.ctx], case, bounds)
    finally:
        for f in contexts.values():
            _defaults(f)
