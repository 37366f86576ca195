"""tests/redzone.py's arena reports what a stray write looks like -- region, side, offsets, length -- and stays silent on a clean run
(no GPU: the arena lives in a CPU tensor or a numpy array).  Also: the case table of tests/test_gpu_footprint.py names every
device-pointer and host-pointer entry point of include/kofft_hip.h."""
import re
from pathlib import Path

import numpy as np
import pytest

import redzone
from redzone import ALIGN, MIN_BAND, Arena, RedzoneError

ROW = 24 * 4  # bytes of one "row" of the planted cases
ROWS = 10


def _arena(device):
    rng = np.random.default_rng(5)
    a = Arena(device, "planted case")
    x = a.input(rng.uniform(-1, 1, (ROWS, 24)).astype(np.float32), align_off=4, row_bytes=ROW, name="x")
    y = a.output(ROWS * ROW, align_off=8, row_bytes=ROW, name="y")
    z = a.inout(rng.uniform(-1, 1, 16).astype(np.float64), align_off=16, name="z")
    return a, x, y, z


def _off(a, r):
    return r.addr - a.base


@pytest.mark.parametrize("device", ["cpu", "host"])
def test_clean_run_passes_and_reads_back(device):
    a, x, y, z = _arena(device)
    want = np.arange(ROWS * 24, dtype=np.float32)
    a.poke(_off(a, y), want)           # the "kernel" writes its whole output
    a.poke(_off(a, z), np.zeros(16))   # and an in-place buffer
    a.verify()
    assert a.read(y, np.float32, (ROWS, 24)).tobytes() == want.tobytes()
    assert a.read(y.addr, np.float32, (ROWS, 24)).tobytes() == want.tobytes()  # by address too
    assert np.all(a.read(z, np.float64, (16,)) == 0)


def test_an_unwritten_output_reads_as_nan():
    a, x, y, z = _arena("cpu")
    assert np.all(np.isnan(a.read(y, np.float32, (ROWS, 24))))


PLANTED = {
    # name: (region, byte offset relative to the region's start (b) or end (e), bytes, expected side, first, last)
    "one byte right before the output": ("y", "b", -1, 1, "before", -1, -1),
    "one byte right after the output": ("y", "e", 0, 1, "after", 0, 0),
    "last byte of the band after the output": ("y", "e", MIN_BAND - 1, 1, "after", MIN_BAND - 1, MIN_BAND - 1),
    "first byte of the band before the input": ("x", "b", -MIN_BAND, 1, "before", -MIN_BAND, -MIN_BAND),
    "a whole extra row after the output": ("y", "e", 0, ROW, "after", 0, ROW - 1),
    "a row one row further": ("y", "e", ROW, ROW, "after", ROW, 2 * ROW - 1),
    "right after the in-place buffer": ("z", "e", 0, 8, "after", 0, 7),
}


@pytest.mark.parametrize("device", ["cpu", "host"])
@pytest.mark.parametrize("plant", list(PLANTED))
def test_planted_writes_are_reported(device, plant):
    name, edge, rel, nbytes, side, first, last = PLANTED[plant]
    a, x, y, z = _arena(device)
    r = {"x": x, "y": y, "z": z}[name]
    at = _off(a, r) + (r.nbytes if edge == "e" else 0) + rel
    a.poke(at, np.full(nbytes, 0x11, np.uint8))  # 0x11 is no byte of the pattern
    with pytest.raises(RedzoneError) as e:
        a.verify()
    assert len(e.value.findings) == 1, str(e.value)
    f = e.value.findings[0]
    assert (f["region"], f["side"], f["first"], f["last"], f["changed"]) == (name, side, first, last, nbytes), str(e.value)
    msg = str(e.value)
    assert "planted case" in msg and f"'{name}'" in msg and side in msg and f"{first:+d}" in msg and f"{nbytes} bytes changed" in msg
    if nbytes == ROW:
        assert f["rows"] == 1 and "a run of 1 rows" in msg


@pytest.mark.parametrize("device", ["cpu", "host"])
def test_one_bit_in_an_input_is_reported(device):
    a, x, y, z = _arena(device)
    byte = a.read(x, np.uint8, (-1,))[37]
    a.poke(_off(a, x) + 37, np.array([byte ^ 0x04], np.uint8))
    with pytest.raises(RedzoneError) as e:
        a.verify("flip")
    f, = e.value.findings
    assert (f["region"], f["side"], f["first"], f["changed"]) == ("x", "input", 37, 1)
    assert "flip" in str(e.value) and "input 'x' was modified" in str(e.value) and "first at byte 37" in str(e.value)


def test_outputs_and_inout_may_change_freely():
    a, x, y, z = _arena("cpu")
    a.poke(_off(a, y), np.zeros(y.nbytes, np.uint8))
    a.poke(_off(a, z), np.ones(z.nbytes, np.uint8))
    a.verify()


def test_layout_keeps_bands_apart_at_every_alignment():
    from test_gpu_footprint import ALIGN_OFFS

    assert set(ALIGN_OFFS) >= {0, 4, 8, 16}
    big_row = 3 * MIN_BAND  # two rows of this exceed the minimum band
    for offs in [(o1, o2, o3) for o1 in ALIGN_OFFS for o2 in ALIGN_OFFS for o3 in ALIGN_OFFS]:
        a = Arena("cpu")
        regs = [a.input(np.zeros(1000, np.uint8), align_off=offs[0], row_bytes=100),
                a.output(2 * big_row, align_off=offs[1], row_bytes=big_row),
                a.output(0, align_off=offs[2]),  # a call that writes nothing
                a.inout(np.zeros(7, np.float32), align_off=offs[0])]
        total = a.layout()
        prev_hi = 0
        for r, off in zip(regs, (offs[0], offs[1], offs[2], offs[0])):
            assert r.start % ALIGN == off
            assert r.lo >= prev_hi, "a band overlaps the neighbour's"
            assert r.start - r.lo >= max(MIN_BAND, 2 * r.row_bytes) and r.hi - (r.start + r.nbytes) >= max(MIN_BAND, 2 * r.row_bytes)
            prev_hi = r.hi
        assert prev_hi <= total
        assert regs[0].addr % ALIGN == offs[0] and a.base % ALIGN == 0
        a.verify()


def test_no_region_after_layout():
    a, x, y, z = _arena("cpu")
    x.addr
    with pytest.raises(RuntimeError):
        a.output(4)


def test_pattern_is_nan_in_both_precisions_and_not_canonical():
    b = redzone.pattern_bytes(64)
    assert np.all(b.view("<u4") == 0x7FF8A5A5)
    assert np.all(np.isnan(b.view(np.float32))) and np.all(np.isnan(b.view(np.float64)))
    assert np.all(np.isnan(redzone.pattern_bytes(64, phase=4).view(np.float64)))  # 8-byte reads at any 4-byte phase
    with np.errstate(invalid="ignore"):
        inf_minus_inf = (np.array([np.inf], np.float32) - np.array([np.inf], np.float32)).view(np.uint32)[0]
    canon = {np.array([np.nan], np.float32).view(np.uint32)[0], np.array([-np.nan], np.float32).view(np.uint32)[0],
             inf_minus_inf, 0x7FC00000, 0xFFC00000}
    assert 0x7FF8A5A5 not in {int(c) for c in canon}
    # an arena's bands hold the pattern in phase with the arena's base, whatever the regions' alignment
    a, x, y, z = _arena("host")
    x.addr
    assert np.all(a.buf[:MIN_BAND].view("<u4") == 0x7FF8A5A5)
    assert np.all(a.buf[y.start + y.nbytes:y.hi].view("<u4") == 0x7FF8A5A5)


# ---- the footprint module's case table covers the header -------------------------------------------------------------------------
HEADER = Path(__file__).resolve().parent.parent / "include" / "kofft_hip.h"
# the multi-device handle needs more than one card to mean anything; its buffers are per device
ALLOWED = {name: "multi-device handle: out of this module's scope (one device)" for name in (
    "kofft_hip_multi_stft_f32_dev", "kofft_hip_multi_fft_c32_dev", "kofft_hip_multi_fft_c64_dev", "kofft_hip_multi_rfft_f32_dev")}
HOST_ENTRIES = """fft_c32 fft_c64 fft_c32_strided fft_c64_strided rfft_f32 rfft_f64 irfft_f32 irfft_f64 dct2_f32 hilbert_f32 cepstrum_f32
dct_direct_f32 dst_direct_f32 dwt_f32 idwt_f32 dwt_multi_f32 idwt_multi_f32 stft_f32 stft_parallel_f32 stft_frame_f32 istft_f32
istft_parallel_f32 istft_frame_f32 stft_magnitudes_f32 fftnd_c32 fftnd_c64""".split()


def _header_functions():
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    return set(re.findall(r"\b(kofft_hip_\w+)\s*\(", text))


def test_every_entry_point_has_a_footprint_case():
    import test_gpu_footprint as fp

    declared = _header_functions()
    dev = {f for f in declared if re.fullmatch(r"kofft_hip_\w+_dev(_oop)?", f)}
    assert len(dev) >= 30
    host = {"kofft_hip_" + h for h in HOST_ENTRIES}
    assert host <= declared, f"not in the header: {sorted(host - declared)}"
    assert all(reason for reason in ALLOWED.values()) and set(ALLOWED) <= dev
    dev_cases = {"kofft_hip_" + c.call for c in fp.DEV_CASES}
    host_cases = {"kofft_hip_" + c.call for c in fp.HOST_CASES}
    assert not (dev_cases | host_cases) - declared, f"cases for calls the header does not declare: {sorted((dev_cases | host_cases) - declared)}"
    missing = sorted(dev - set(ALLOWED) - dev_cases)
    assert not missing, f"device-pointer entry points without a footprint case: {missing}"
    missing = sorted(host - host_cases)
    assert not missing, f"host-pointer entry points without a footprint case: {missing}"
    # every case has a driver
    assert {c.call for c in fp.DEV_CASES} <= set(fp.DEV_DRIVERS) and {c.call for c in fp.HOST_CASES} <= set(fp.HOST_DRIVERS)
